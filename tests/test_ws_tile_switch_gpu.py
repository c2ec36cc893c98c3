"""-m gpu: the halo waves' tile switch of conv_fprop_ws_kernel (fprop_dma.hip: set_fetch_tile) -- tile index -> (image, tile row,
tile column) through the launcher's multiplier / shift pairs, the border test of a halo piece as two packed 16-bit operations,
the virtual concat's low-resolution offsets and the output pixel table from per-lane constants.

Geometries at which a wrong (n, hb, wb), a wrong border range or a wrong offset shows:

  carries          N = 3, 48 x 32, 64 -> 64 on 2 % of the CUs: a 3 x 2 tile grid, several tiles per persistent block, carries from tile
                   column to tile row to image
  partial tiles    N = 1, 20 x 24, 64 -> 40
  two chunks       N = 2, 28 x 28, 128 -> 64 on 16 x 16 tiles (fprop_dma_cfg 1) and on 14 x 14 tiles (3): the switch in front of a
                   tile's last chunk, the 14 x 14 row mapping of the pixel table
  virtual concat   N = 2, 16 x 16 with u at 8 x 8, 64 + 64 -> 64: the offsets into u
  plane gather     N = 2, data gradient of an up segment, low resolution 16 x 16, 64 and 32 dy channels: four planes, and the
                   two-planes-per-chunk form

Every case launches its random operands first (fresh tensors; the first launch of the geometry in this module): outputs within the
derived bound of tests/errbound.py around float64, forward statistics summed over the replicas equal to the float64 sums of the
stored output to 1e-6 relative (operands with a bias of about one).  Then impulse operands -- single non-zero pixels at image
corners, on both sides of the tile seams, on a tile edge and in the last image, so that every output is one product -- must
give the float64 result exactly."""
import pytest
import torch
import torch.nn.functional as F

import errbound as eb
import fused_errbound as fe
from segnb import _native as nv
from segnb.engine import PackTable, Runtime, UpCatConvOp, View
from test_ws_epi_gpu import UPD, _check_bounds, _check_stats, _launch_plain, _nhwc, _plain_case, _rand, _upd_case, knobs

pytestmark = pytest.mark.gpu

# name: (N, H, W, Ci, Co, conv_cu_pct or None, fprop_dma_cfg or None, tile side)
PLAIN = {
    'carries 48x32 64->64 5 CUs': (3, 48, 32, 64, 64, 2, None, 16),
    'partial tiles 20x24 64->40': (1, 20, 24, 64, 40, None, None, 16),
    'two chunks 28x28 128->64 cfg 1': (2, 28, 28, 128, 64, None, 1, 16),
    'two chunks 28x28 128->64 cfg 3': (2, 28, 28, 128, 64, None, 3, 14),
}


def probe_pixels(N, H, W, T):
    """(n, r, c), pairwise at least 3 apart inside an image: the image corners of the first image, both sides of the first tile
    seam's corner, a pixel on a tile's edge in its row and one in its column, the same seam in a middle image, and in the LAST
    image its far corner, the seam corner and the first pixel"""
    want = [(0, 0, 0), (0, 0, W - 1), (0, H - 1, 0), (0, H - 1, W - 1)]
    if H > T and W > T:
        want += [(0, T - 1, T - 1), (0, T + 2, T + 2), (0, T, 5), (0, 5, T), (0, T - 1, W - 1 - 3)]
    last = N - 1
    mid = N // 2
    if mid not in (0, last) and H > T:
        want += [(mid, T, T - 1), (mid, T - 4, T), (mid, H - 1, W - 1), (mid, 0, 0)]
    if last > 0:
        want += [(last, H - 1, W - 1), (last, 0, 0), (last, min(T, H - 1) - 1, min(T, W - 1)), (last, min(T, H - 1) + 3, min(T, W - 1) - 1)]
    out = []
    for n, r, c in want:
        if 0 <= r < H and 0 <= c < W and all(m != n or max(abs(r - r2), abs(c - c2)) >= 3 for m, r2, c2 in out):
            out.append((n, r, c))
    return out


def probe_tensor(N, C, H, W, pixels, shift=0):
    """zero but for one impulse 2^j (j cycling over -2..2, alternating sign) per pixel, each in a channel of its own"""
    t = torch.zeros(N, C, H, W)
    for i, (n, r, c) in enumerate(pixels):
        t[n, (7 * i + shift) % C, r, c] = 2.0 ** ((i + shift) % 5 - 2) * (-1) ** i
    return t


def test_probe_pixels_reach_seams_and_the_last_image():
    px = probe_pixels(3, 48, 32, 16)
    assert (0, 0, 0) in px and (0, 15, 15) in px and (0, 18, 18) in px and (0, 16, 5) in px and (2, 47, 31) in px and (1, 16, 15) in px
    assert len(px) >= 12
    px = probe_pixels(2, 28, 28, 14)
    assert (0, 13, 13) in px and (0, 16, 16) in px and (1, 27, 27) in px


@pytest.mark.parametrize('name', sorted(PLAIN))
def test_tile_switch_forward_and_data_gradient(name):
    N, H, W, Ci, Co, cu_pct, cfg, T = PLAIN[name]
    w, b, x, dy, r = _plain_case(name, N, H, W, Ci, Co)
    y, st, dx, census = _launch_plain(w, b, x, dy, None, cu_pct, cfg)          # cold: random operands first
    assert census.get('kernel:fprop_dma') in (1, 2), census                      # (a data gradient of Co % 64 != 0 input channels runs elsewhere)
    if cfg == 3:
        assert census.get('tile:ws14') == 2, census
    msgs = []
    _check_bounds(name, msgs, y, dx, r, Ci, Co)
    _check_stats(name, msgs, st, y, Co)
    px = probe_pixels(N, H, W, T)
    xi, dyi = probe_tensor(N, Ci, H, W, px), probe_tensor(N, Co, H, W, px, shift=3)
    yi, _, dxi, _ = _launch_plain(w, b, xi, dyi, None, cu_pct, cfg)
    msgs.append(eb.mismatches(name + ': impulse forward', yi[..., :Co].float().permute(0, 3, 1, 2), eb.impulse_expect_y(xi, w, b, 1, 1, False, 'bf16')))
    msgs.append(eb.mismatches(name + ': impulse data gradient', dxi[..., :Ci].float().permute(0, 3, 1, 2),
                              eb.impulse_expect_dx(xi, w, dyi, 1, 1, False, 'bf16')))
    msgs = [m for m in msgs if m]
    assert not msgs, '\n'.join(msgs)


# ------------------------------------------------------------------------------------------------ virtual concat
VCAT = (2, 16, 64, 64, 64)      # N, S, Cu, Cs, Co


def _launch_vcat(w, b, u, sk):
    """the virtual-concat forward with statistics: u [N,Cu,S/2,S/2] is read in place of the upsampled channels, which hold garbage"""
    N, S, Cu, Cs, Co = VCAT
    rt = Runtime('cuda', 'bf16')
    op = UpCatConvOp(rt, w.cuda(), b.cuda(), [(Cu, Cu), (Cs, Cs)], need_dgrad=True)
    PackTable(rt, op.full.pack_jobs(S, S), 'segnb_pack_weight_multi', 'segnb_pack_weight').run()
    cat = View.alloc(rt, N, S, S, Cu + Cs)
    cat.t.fill_(5.0)
    cat.dense()[..., Cu:] = _nhwc(sk, rt)
    uv, duv = View.alloc(rt, N, S // 2, S // 2, Cu), View.alloc(rt, N, S // 2, S // 2, Cu)
    uv.dense().copy_(_nhwc(u, rt))
    op.bind_up(uv, duv)
    assert op.virtual(N, S, S)
    yv, stats = View.alloc(rt, N, S, S, op.Cop), rt.zeros((16, 2, op.Cop), torch.float64)
    yv.t.fill_(3.0)
    torch.cuda.synchronize()
    with knobs(call_census=1):
        nv.census_read()
        op.fprop(cat, yv, stats)
        census = nv.census_read()
    torch.cuda.synchronize()
    return yv.dense().contiguous().cpu(), stats.cpu(), census


def test_tile_switch_virtual_concat_forward():
    N, S, Cu, Cs, Co = VCAT
    name = 'virtual concat 16x16 64+64->64'
    gen = torch.Generator().manual_seed(eb.seed_of(name))
    w = _rand((Co, Cu + Cs, 3, 3), gen, (2.0 / ((Cu + Cs) * 9)) ** 0.5)
    b = 1.0 + 0.1 * torch.randn(Co, generator=gen)
    u, sk = _rand((N, Cu, S // 2, S // 2), gen), _rand((N, Cs, S, S), gen)
    up = lambda t: F.interpolate(t, scale_factor=2, mode='nearest')
    y, st, census = _launch_vcat(w, b, u, sk)                                    # cold
    assert census.get('segnb_conv_fprop_upcat') == 1 and census.get('epi:1') == 1, census      # (served by conv_fprop_ws_kernel)
    r = eb.conv_refs(torch.cat([up(u), sk], 1), w, b, torch.zeros(N, Co, S, S), 1, 1, False)
    msgs = []
    worst, m = eb.within_bound(name + ' y', y[..., :Co].float().permute(0, 3, 1, 2), r['y'], r['mag_y'], r['K_y'], 'bf16')
    print('%s: y worst err / bound %.3f' % (name, worst))
    msgs.append(m)
    _check_stats(name, msgs, st, y, Co)
    # impulses on u 3 apart on the LOW-resolution grid (a 3 x 3 window holds at most one of the 2 x 2 blocks they become) and on
    # the skip tensor, weights on a 1/64 grid: the up to four products behind an output add exactly in fp32 in every order
    wg = fe.grid_weights(VCAT)
    for pas in (0, 4):
        ui, ski = fe.shifted_impulses(N, Cu, S // 2, S // 2, 3, pas), fe.shifted_impulses(N, Cs, S, S, 3, pas)
        yi, _, _ = _launch_vcat(wg, b, ui, ski)
        want = eb._conv64(torch.cat([up(ui), ski], 1).double(), wg.double(), None, 1, 1, False)
        want = eb.round_out(fe._exact32(want) + b.float()[None, :, None, None], 'bf16')
        msgs.append(eb.mismatches('%s: impulses, pass %d' % (name, pas), yi[..., :Co].float().permute(0, 3, 1, 2), want))
    msgs = [m for m in msgs if m]
    assert not msgs, '\n'.join(msgs)


# ------------------------------------------------------------------------------------------------ plane gather
def _launch_upd(name, w, dy):
    """the data gradient of the up segment: du [N,S/2,S/2,Cu] from dy [N,Co,S,S] through the 4 x 4 / stride-2 plane gather"""
    N, S, Cu, Cs, Co, _ = UPD[name]
    rt = Runtime('cuda', 'bf16')
    op = UpCatConvOp(rt, w.cuda(), None, [(Cu, Cu), (Cs, Cs)], need_dgrad=True)
    PackTable(rt, op.up.pack_jobs(S // 2, S // 2), 'segnb_pack_weight_multi', 'segnb_pack_weight').run()
    dyv = View.alloc(rt, N, S, S, op.Cop)
    dyv.dense()[..., :Co] = _nhwc(dy, rt)
    duv = View.alloc(rt, N, S // 2, S // 2, Cu)
    duv.t.fill_(7.0)
    torch.cuda.synchronize()
    with knobs(call_census=1):
        nv.census_read()
        op.up.dgrad(dyv, duv)
        census = nv.census_read()
    torch.cuda.synchronize()
    return duv.dense().contiguous().cpu(), census


@pytest.mark.parametrize('name', ['16->32 64+64->64', '16->32 64+64->32'])
def test_tile_switch_plane_gather_data_gradient(name):
    N, S, Cu, Cs, Co, _ = UPD[name]
    w, dy, du_ref, du_mag = _upd_case(name)
    du, census = _launch_upd(name, w, dy)                                        # cold
    assert census.get('kernel:fprop_dma') == 1, census
    msgs = []
    worst, m = eb.within_bound(name + ' du', du.float().permute(0, 3, 1, 2), du_ref, du_mag, Co * 16, 'bf16')
    print('%s: du worst err / bound %.3f' % (name, worst))
    msgs.append(m)
    # dy impulses 4 apart: every element of du is one product with a rounded phase weight
    wt = fe.phase_weights(w[:, :Cu])
    for pas in (0, 5, 15):
        dyi = fe.shifted_impulses(N, Co, S, S, 4, pas)
        dui, _ = _launch_upd(name, w, dyi)
        us = torch.zeros(N, Cu, S // 2, S // 2, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(us, wt, None, stride=2, padding=1).backward(dyi.double())
        msgs.append(eb.mismatches('%s: impulses, pass %d' % (name, pas), dui.float().permute(0, 3, 1, 2), fe.bf(fe._exact32(us.grad))))
    msgs = [m for m in msgs if m]
    assert not msgs, '\n'.join(msgs)
