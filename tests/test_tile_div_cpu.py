"""CPU-only: the multiplier / shift division of csrc/tile_div.h (the halo waves' tile switch of conv_fprop_ws_kernel: tile index ->
image, tile row, tile column) against / and %.

The header is plain C++; a stand-alone host program built here with the host compiler includes it and compares, for every divisor
the launchers can produce on images of 7..1024 pixels with 8-, 14-, 16- and 32-pixel tiles -- WB = ceil(S / t) and HB * WB =
ceil(S / r) * ceil(S / t) for every pair (r, t): the tile grids of the ZF_UNET, LinkNet34, UNet16 and FCDenseNet launches are among
them -- EVERY numerator from 0 to TILE_DIV_MAX, the bound beyond which the launchers decline: quotient with /, remainder with %.
Beyond that bound the range the header proves (numerators below 2^30, divisors below 2^30) is sampled at its edges."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'segmentation-networks-benchmark_amd', 'csrc')
TILES = (8, 14, 16, 32)

PROGRAM = r'''
#include "tile_div.h"
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

static_assert(tile_div(7, tile_div_make(1)) == 7 && tile_div(100, tile_div_make(7)) == 14, "usable in constant expressions");

// first numerator in [0, last] whose quotient or remainder differs from / and %, or -1
static long long first_bad(uint32_t d, uint32_t last) {
    const TileDiv m = tile_div_make(d);
    for (uint32_t n = 0;; ++n) {
        const uint32_t q = tile_div(n, m), r = n - q * d;
        if (q != n / d || r != n % d) return n;
        if (n == last) return -1;
    }
}

int main(int argc, char** argv) {
    std::printf("max %u\n", TILE_DIV_MAX);
    std::vector<uint32_t> ds;
    for (int i = 1; i < argc; ++i) ds.push_back((uint32_t)std::strtoul(argv[i], nullptr, 10));
    std::atomic<size_t> next{0};
    std::atomic<int> bad{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < 4; ++t)
        pool.emplace_back([&] {
            for (size_t i = next++; i < ds.size(); i = next++) {
                const long long n = first_bad(ds[i], TILE_DIV_MAX);
                if (n >= 0) {
                    std::printf("BAD exhaustive d=%u n=%lld\n", ds[i], n);
                    ++bad;
                }
            }
        });
    for (auto& th : pool) th.join();
    std::printf("exhaustive %zu divisors\n", ds.size());
    // the edges of the proven range: numerators just below 2^30 and around the multiples of d, small, large and power-of-two divisors
    const uint32_t top = (1u << 30) - 1;
    size_t sampled = 0;
    std::vector<uint32_t> wide = {1, 2, 3, 5, 7, 255, 256, 257, 16383, 16384, 16385, 65535, 65536, 65537, 1000003, (1u << 29) - 1, 1u << 29,
                                  (1u << 29) + 1, (1u << 30) - 1};
    for (uint32_t d : ds) wide.push_back(d);
    for (uint32_t d : wide) {
        const TileDiv m = tile_div_make(d);
        for (uint32_t k = 0; k < 4096; ++k) {
            const uint32_t near_top = top - k;
            const uint32_t mult = (top / d - (k < top / d ? k : 0)) * d;      // a multiple of d, and its two neighbours
            for (uint32_t n : {near_top, mult, mult - (mult ? 1u : 0u), mult + 1 <= top ? mult + 1 : mult}) {
                ++sampled;
                if (tile_div(n, m) != n / d) {
                    std::printf("BAD sampled d=%u n=%u\n", d, n);
                    ++bad;
                }
            }
        }
    }
    std::printf("sampled %zu\n", sampled);
    return bad.load() ? 1 : 0;
}
'''


def divisors():
    out = set()
    for s in range(7, 1025):
        for t in TILES:
            out.add(-(-s // t))
            for r in TILES:
                out.add(-(-s // r) * -(-s // t))
    return sorted(out)


def test_divisor_set_covers_the_step():
    ds = divisors()
    assert ds[0] == 1 and ds[-1] == 128 * 128
    # ZF_UNET 224^2 (16 x 16 and 14 x 14 tiles), 1024^2 inputs, the non-square grid of the 8 x 32 tile
    for d in (1, 4, 14, 16, 49, 196, 256, 28 * 7, 64 * 64, 128 * 32):
        assert d in ds, d


def test_tile_div_is_exact_up_to_the_launchers_bound(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    src, exe = tmp_path / 'tile_div_check.cpp', tmp_path / 'tile_div_check'
    src.write_text(PROGRAM)
    subprocess.run([cxx, '-O2', '-std=c++17', '-pthread', '-I', CSRC, str(src), '-o', str(exe)], check=True)
    ds = divisors()
    r = subprocess.run([str(exe)] + [str(d) for d in ds], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.split('\n')
    assert 'exhaustive %d divisors' % len(ds) in lines
    bound = int(lines[0].split()[1])
    # the bound leaves room for every launch a 32-bit buffer descriptor can hold: a bs = 32 batch of 1024 x 1024 images in 14 x 14
    # tiles is 32 * 74 * 74 = 175 232 tiles
    assert bound >= 8 * 32 * 74 * 74 and bound < 1 << 30


def test_launchers_decline_beyond_the_bound():
    """every launcher of conv_fprop_ws_kernel that walks a tile grid sets the pairs through ws_tile_div, which refuses a tile count
    (look-ahead included) beyond TILE_DIV_MAX; the kernel itself divides nowhere by the grid"""
    text = open(os.path.join(CSRC, 'fprop_dma.hip')).read()
    # launch_ws_row, the launcher of every table row: the grid comes from ws_tile_grid, and a refusal declines the launch ...
    assert len(re.findall(r'if \(!ws_tile_grid<C>\(a, [^;]*\)\) return SEGNB_LAUNCH_DECLINED;', text)) == 1
    assert len(re.findall(r'\bws_tile_grid<', text)) == 1 and len(re.findall(r'hipLaunchKernelGGL\(', text)) == 1
    assert text.index('if (!ws_tile_grid<C>(') < text.index('hipLaunchKernelGGL(')
    assert len(re.findall(r'\ba\.GM\s*=\s*gm;', text)) == 1 and len(re.findall(r'\ba\.HB\s*=', text)) == 1
    # ... which is ws_tile_div's, for every form but the tall one (no tile grid: it walks virtual rows)
    grid = text[text.index('bool ws_tile_grid(WsArgs& a, int ntl, int cus) {'):text.index('int launch_ws_row(')]
    assert 'return C::TALL || ws_tile_div(a);' in grid and grid.index('a.GM = gm;') < grid.index('ws_tile_div(a)')
    assert '2ll * a.GM > (long long)TILE_DIV_MAX) return false;' in text
    kernel = text[text.index('void conv_fprop_ws_kernel('):text.index('int ksplit_workspace(')]
    for spelled in ('/ a.WB', '/ (a.HB', '% a.WB'):
        assert spelled not in kernel, spelled
