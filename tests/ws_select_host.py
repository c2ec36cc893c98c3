"""csrc/ws_select.h asked from Python: a stand-alone host program, built with the host compiler alone, that includes the header and
prints what ws_select / rw_select answer for a list of launches (tests/test_ws_tile14_cpu.py, tests/test_conv_select_gpu.py)."""
import os
import shutil
import subprocess
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'segmentation-networks-benchmark_amd', 'csrc')

PROGRAM = r'''
#include "ws_select.h"
#include <cstdio>
#include <cstring>

static_assert(WS_TILES[WS_14x14].BM == 224 && WS_TILES[WS_TALL].TALL && !WS_TILES[WS_TALL].MF16, "the table is a constant expression");

// one query per line of the file argv[1]:
//   ws N H W Hi Wi Ci Co stats mask ep upcat dbg row_major window no_prev bias  dma upd mask cfg epi ksplit nostats cus levels14
//        -> row form epi ks ks_form tag BM
//   rw Co NCH Wo stats  -> row BN NS NSW R WT
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* in = std::fopen(argv[1], "r");
    if (in == nullptr) return 2;
    char kind[8];
    while (std::fscanf(in, "%7s", kind) == 1) {
        if (std::strcmp(kind, "ws") == 0) {
            int v[25];
            for (int& x : v)
                if (std::fscanf(in, "%d", &x) != 1) return 3;
            WsFacts f = {v[0], v[1], v[2], v[3], v[4], v[5], v[6]};
            f.stats = v[7]; f.mask = v[8]; f.ep = v[9]; f.upcat = v[10]; f.dbg = v[11]; f.row_major = v[12];
            f.window = v[13]; f.no_prev = v[14]; f.bias = v[15];
            const WsKnobs k = {v[16] != 0, v[17] != 0, v[18] != 0, v[19], v[20], v[21], v[22], v[23], (unsigned)v[24]};
            const WsChoice c = ws_select(f, k);
            std::printf("%d %d %d %d %d %s %d\n", c.row, c.form, (int)c.epi, c.ks, c.ks_form, c.row < 0 ? "-" : WS_TILES[c.row].tag,
                        c.row < 0 ? 0 : WS_TILES[c.row].BM);
        } else if (std::strcmp(kind, "rw") == 0) {
            int Co, NCH, Wo, stats;
            if (std::fscanf(in, "%d %d %d %d", &Co, &NCH, &Wo, &stats) != 4) return 3;
            const int r = rw_select(Co, NCH, Wo, stats != 0);
            const RwTile t = r < 0 ? RwTile{0, 0, 0, 0, 0} : RW_TILES[r];
            std::printf("%d %d %d %d %d %d\n", r, t.BN, t.NS, t.NSW, t.R, t.WT);
        } else {
            return 3;
        }
    }
    std::fclose(in);
    return 0;
}
'''

# rows, forms and windows of ws_select.h, by their enumerators' values
ROWS = ('8x32', '16x16', 'tall', '14x14', 'upd 8x32', 'upd 16x16', 'upf 8x32', 'upf 16x16')
STATS, NOSTATS, MASK, EP, DBG, KS_STATS, KS_NOSTATS = range(7)
WIN_3x3, WIN_UPD, WIN_UPF = range(3)

Choice = namedtuple('Choice', 'row form epi ks ks_form tag BM')
KNOB_DEFAULTS = dict(dma=1, upd=1, kmask=1, cfg=-1, epi=-1, ksplit=1, nostats=1, cus=256, levels14=7)


def ws_query(N, H, W, Ci, Co, Hi=None, Wi=None, stats=False, mask=False, ep=False, upcat=False, dbg=False, row_major=True,
             window=WIN_3x3, no_prev=False, bias=False, **knobs):
    """one 'ws' line; knobs: KNOB_DEFAULTS' names"""
    k = dict(KNOB_DEFAULTS, **knobs)
    assert sorted(k) == sorted(KNOB_DEFAULTS), knobs
    Hi, Wi = (H if Hi is None else Hi), (W if Wi is None else Wi)
    facts = (N, H, W, Hi, Wi, Ci, Co, stats, mask, ep, upcat, dbg, row_major, window, no_prev, bias)
    return 'ws ' + ' '.join(str(int(v)) for v in facts + tuple(k[n] for n in ('dma', 'upd', 'kmask', 'cfg', 'epi', 'ksplit', 'nostats',
                                                                            'cus', 'levels14')))


def rw_query(Co, NCH, Wo, stats):
    return 'rw %d %d %d %d' % (Co, NCH, Wo, int(stats))


def build(tmp_path, flags=()):
    """-> path of the program, compiled in tmp_path with the host C++ compiler (and the extra flags)"""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    src, exe = os.path.join(str(tmp_path), 'ws_select_check.cpp'), os.path.join(str(tmp_path), 'ws_select_check')
    with open(src, 'w') as f:
        f.write(PROGRAM)
    subprocess.run([cxx, '-O1', '-std=c++17', '-Wall', '-Werror', '-I', CSRC, src, '-o', exe] + list(flags), check=True)
    return exe


def ask(exe, queries, tmp_path):
    """the program's answers, in the order of the queries: Choice (row None where declined) for 'ws', (row or None, tile) for 'rw'"""
    path = os.path.join(str(tmp_path), 'queries.txt')
    with open(path, 'w') as f:
        f.write('\n'.join(queries) + '\n')
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = r.stdout.strip().split('\n')
    assert len(lines) == len(queries), (len(lines), len(queries))
    out = []
    for q, line in zip(queries, lines):
        v = line.split()
        if q.startswith('ws'):
            row = int(v[0])
            out.append(Choice(None if row < 0 else row, int(v[1]), bool(int(v[2])), int(v[3]), int(v[4]), v[5], int(v[6])))
        else:
            row = int(v[0])
            out.append((None if row < 0 else row, tuple(int(x) for x in v[1:])))
    return out
