"""-m gpu: conv_fprop_ws_kernel with the previous tile's store rows on peeled, straight-line taps (segnb_tune
"fprop_dma_epi" = 1, the WsEpi instantiations: which tap carries a row is a compile-time fact; the row runs behind the tap's
last MFMA as in the plain order, one tap body for both) against the plain order (knob 0) and against float64.

Every geometry runs under knob 1 first -- fresh tensors, the first launch of that geometry in the test: a counted wait that misses
a read shows on a cold launch only -- then under knob 1 again, then under knob 0:

  * the stored outputs (y, dx, dz, du) of knob 1 are the bits of knob 0 and of its own second run;
  * the forward's statistics are the bits of knob 0 REPLICA BY REPLICA, all 16 (same blocks, same threads, same order);
  * the outputs lie within the derived bound of tests/errbound.py around the float64 convolution on the CPU;
  * the statistics, summed over the replicas, are the float64 sum and sum of squares of the STORED y to 1e-6 relative (operands
    with a bias of about one, so that the sums are well conditioned);
  * the launches were served by the new order (the call census counts "epi:1" beside "kernel:fprop_dma").

Geometries whose instantiation keeps the plain order (split K, the tall 7 x 7 form, the 2 x 2-window plane gather of an up
segment) run under knob 1 without "epi:1" in the census and keep their bits."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import errbound as eb
import fused_errbound as fe
from segnb import _native as nv
from segnb import convplan as cp
from segnb.engine import ConvOp, PackTable, Runtime, UpCatConvOp, View

pytestmark = pytest.mark.gpu

# name: (N, H, W, Ci, Co, conv_cu_pct or None, fprop_dma_cfg or None)
PLAIN = {
    # one chunk per tile: store rows ride on 8 of its 9 taps; 8 tiles on 2 % of the CUs (5 of 256): 2, 2, 2, 1, 1 tiles per
    # persistent block -- the rows pending across tiles and the drain behind the last tile
    '32x32 64->64 5 CUs': (2, 32, 32, 64, 64, 2, None),
    # two chunks, four tiles per image: the 14 x 14 row mapping (cfg 3) and the halo double buffer across tiles
    '28x28 128->64 cfg 1': (2, 28, 28, 128, 64, None, 1),
    '28x28 128->64 cfg 3': (2, 28, 28, 128, 64, None, 3),
    '14x14 128->192': (3, 14, 14, 128, 192, None, None),      # three channel tiles, one tile per image
    # partial tiles, and channel chunks past Co in the last channel tile: dummy rows neither stored nor counted
    '20x24 64->40': (1, 20, 24, 64, 40, None, None),
}
STAT_RTOL = 1e-6


class knobs(object):
    """segnb_tune settings for a block, back at their defaults afterwards"""
    DEFAULTS = {'fprop_dma_epi': -1, 'fprop_dma_cfg': -1, 'conv_cu_pct': 100, 'call_census': 0, 'fprop_ksplit': 1, 'fprop_dma_dbg': 0}

    def __init__(self, **kv):
        self.kv = {k: v for k, v in kv.items() if v is not None}

    def __enter__(self):
        try:
            for k, v in self.kv.items():
                nv.call('segnb_tune', k.encode(), v)
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *a):
        for k in self.kv:
            nv.call('segnb_tune', k.encode(), self.DEFAULTS[k])


def _rand(shape, gen, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).bfloat16().float()


def _nhwc(t, rt):
    return t.permute(0, 2, 3, 1).contiguous().to('cuda', rt.tdtype)


def _bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16)) if a.dtype == torch.bfloat16 else torch.equal(a, b)


@functools.lru_cache(maxsize=None)
def _plain_case(name, N, H, W, Ci, Co):
    """operands (bf16-exact) and the float64 references of a 3 x 3 / pad 1 convolution, computed once per geometry"""
    gen = torch.Generator().manual_seed(eb.seed_of(name))
    w = _rand((Co, Ci, 3, 3), gen, (2.0 / (Ci * 9)) ** 0.5)
    b = 1.0 + 0.1 * torch.randn(Co, generator=gen)
    x, dy = _rand((N, Ci, H, W), gen), _rand((N, Co, H, W), gen)
    return w, b, x, dy, eb.conv_refs(x, w, b, dy, 1, 1, False)


def _read_stamps():
    """the in-kernel stamps of the last stamped launch's block 0: [role][step][4] shader clocks (role 0 = matrix wave 0)"""
    buf = (ctypes.c_ulonglong * (3 * 256 * 4))()
    nv.call('segnb_debug_stamps', ctypes.cast(buf, ctypes.c_void_p))
    return np.array(buf[:], dtype=np.uint64).reshape(3, 256, 4)


def _launch_plain(w, b, x, dy, epi, cu_pct=None, cfg=None, ksplit=None, dbg=None, stamps=None):
    """forward with statistics and data gradient on FRESH tensors under fprop_dma_epi = epi
    -> raw bf16 y [N,H,W,Cop], statistics [16,2,Cop] (every replica), raw bf16 dx, census of the two launches
    (dbg: segnb_tune "fprop_dma_dbg" for the two launches; stamps: a list that takes the stamps read behind each of them)"""
    N, Ci, H, W = x.shape
    Co = w.shape[0]
    rt = Runtime('cuda', 'bf16')
    op = ConvOp(rt, w.cuda(), b.cuda(), [(Ci, cp.pad8(Ci))], 1, 1, False, need_dgrad=True)
    op.pack(H, W)
    xv, dyv = View.alloc(rt, N, H, W, op.Cip), View.alloc(rt, N, H, W, op.Cop)
    xv.dense()[..., :Ci] = _nhwc(x, rt)
    dyv.dense()[..., :Co] = _nhwc(dy, rt)
    yv, dxv = View.alloc(rt, N, H, W, op.Cop), View.alloc(rt, N, H, W, op.Cip)
    yv.t.fill_(3.0)
    dxv.t.fill_(3.0)
    stats = rt.zeros((16, 2, op.Cop), torch.float64)
    torch.cuda.synchronize()
    with knobs(fprop_dma_epi=epi, fprop_dma_cfg=cfg, conv_cu_pct=cu_pct, fprop_ksplit=ksplit, fprop_dma_dbg=dbg, call_census=1):
        nv.census_read()
        for launch in (lambda: op.fprop(xv, yv, stats), lambda: op.dgrad(dyv, dxv)):
            launch()
            if stamps is not None:
                torch.cuda.synchronize()
                stamps.append(_read_stamps())
        census = nv.census_read()
    torch.cuda.synchronize()
    return yv.dense().contiguous().cpu(), stats.cpu(), dxv.dense().contiguous().cpu(), census


def _check_stats(name, msgs, st, y_raw, Co):
    v = y_raw.double().reshape(-1, y_raw.shape[-1])[:, :Co]
    for row, what, tot in ((0, 'sum', v.sum(0)), (1, 'sum of squares', (v * v).sum(0))):
        rel = ((st.sum(0)[row, :Co] - tot).abs() / tot.abs()).max()
        print('%s: statistics %s, worst relative difference from the float64 sum of the stored y %.3g' % (name, what, float(rel)))
        if not bool(rel <= STAT_RTOL):
            msgs.append('%s: %s of the epilogue differs from the stored y by %.3g relative (> %g)' % (name, what, float(rel), STAT_RTOL))


def _check_bounds(name, msgs, y_raw, dx_raw, r, Ci, Co):
    for what, got, ref, mag, K, C in (('y', y_raw, r['y'], r['mag_y'], r['K_y'], Co), ('dx', dx_raw, r['dx'], r['mag_dx'], r['K_dx'], Ci)):
        worst, m = eb.within_bound('%s %s' % (name, what), got[..., :C].float().permute(0, 3, 1, 2), ref, mag, K, 'bf16')
        print('%s: %s worst err / bound %.3f' % (name, what, worst))
        msgs.append(m)


def _same(name, msgs, what, a, b, versus):
    if not _bits(a, b):
        bad = a != b
        msgs.append('%s: %s differs from %s in %d/%d elements, first %s' % (name, what, versus, int(bad.sum()), bad.numel(),
                                                                             bad.nonzero()[:4].tolist()))


@pytest.mark.parametrize('name', sorted(PLAIN))
def test_epi_forward_and_data_gradient(name):
    N, H, W, Ci, Co, cu_pct, cfg = PLAIN[name]
    w, b, x, dy, r = _plain_case(name, N, H, W, Ci, Co)
    y1, st1, dx1, c1 = _launch_plain(w, b, x, dy, 1, cu_pct, cfg)          # cold: the first launches of this geometry, fresh tensors
    y1b, st1b, dx1b, _ = _launch_plain(w, b, x, dy, 1, cu_pct, cfg)
    y0, st0, dx0, c0 = _launch_plain(w, b, x, dy, 0, cu_pct, cfg)
    served = c1.get('kernel:fprop_dma')
    assert served in (1, 2) and c1.get('epi:1') == served, c1        # (a data gradient of Co % 64 != 0 input channels runs elsewhere)
    assert 'epi:1' not in c0 and c0.get('kernel:fprop_dma') == served, c0
    if cfg == 3:
        assert c1.get('tile:ws14') == 2, c1
    msgs = []
    for what, a, ref, ref2 in (('y', y1, y0, y1b), ('dx', dx1, dx0, dx1b), ('statistics (16 replicas)', st1, st0, st1b)):
        _same(name, msgs, what, a, ref, 'the plain order')
        _same(name, msgs, what, a, ref2, 'its own second launch')
    _check_bounds(name, msgs, y1, dx1, r, Ci, Co)
    _check_stats(name + ' knob 1', msgs, st1, y1, Co)
    msgs = [m for m in msgs if m]
    assert not msgs, '\n'.join(msgs)


# ------------------------------------------------------------------------------------------------ timing instantiations
@pytest.mark.parametrize('epi', [1, 0])
def test_stamped_timing_instantiation_keeps_the_bits(epi):
    """segnb_tune "fprop_dma_dbg" = 32 (stamps only, nothing removed) runs the DBG instantiations -- of WsEpi under knob 1, of the
    plain order under knob 0 -- on several tiles per persistent block with rows pending across tiles: the outputs and every
    statistics replica are the bits of the fprop_dma_dbg = 0 run, and matrix wave 0 of block 0 left its four stamps (tap start,
    MFMAs issued, store row issued, past the barrier) on every tap of its first tile, non-zero and non-decreasing"""
    name = '32x32 64->64 5 CUs'
    N, H, W, Ci, Co, cu_pct, cfg = PLAIN[name]
    w, b, x, dy, _ = _plain_case(name, N, H, W, Ci, Co)
    y0, st0, dx0, c0 = _launch_plain(w, b, x, dy, epi, cu_pct, cfg)
    before, stamps = _read_stamps(), []
    y1, st1, dx1, c1 = _launch_plain(w, b, x, dy, epi, cu_pct, cfg, dbg=32, stamps=stamps)
    assert c1 == c0 and c1.get('kernel:fprop_dma') == 2 and c1.get('epi:1', 0) == 2 * epi, (c1, c0)
    msgs = []
    for what, a, ref in (('y', y1, y0), ('dx', dx1, dx0), ('statistics (16 replicas)', st1, st0)):
        _same(name, msgs, what, a, ref, 'the fprop_dma_dbg = 0 run')
    ntaps = (Ci // 64) * 9          # the first tile of block 0: steps 0 .. ntaps - 1 of the matrix role
    for what, st in zip(('forward', 'data gradient'), stamps):
        m = st[0, :ntaps].astype(np.int64)
        print('%s knob %d %s: stamps of the first tile relative to its start\n%s' % (name, epi, what, m - m[0, 0]))
        if not (m != 0).all():
            msgs.append('%s: a stamp of the first tile is zero' % what)
        if not (np.diff(m, axis=1) >= 0).all():
            msgs.append('%s: the four stamps of a tap decrease' % what)
        if not (st[0, :ntaps] != before[0, :ntaps]).all():
            msgs.append('%s: the launch left a stamp of the first tile as it found it' % what)
        before = st
    assert not msgs, '\n'.join(msgs)


# ------------------------------------------------------------------------------------------------ activation mask
def _launch_mask(epi):
    """UNet16's form, conv + ReLU without BatchNorm: the data gradient stores dz = g * act'(a1) and sums it per channel"""
    N, H, W, C1, C2, act = 2, 16, 16, 64, 64, nv.ACT_RELU
    rt = Runtime('cuda', 'bf16')
    gen = torch.Generator().manual_seed(eb.seed_of('epi mask 16x16 64->64'))
    w2 = _rand((C2, C1, 3, 3), gen, (2.0 / (C1 * 9)) ** 0.5)
    dy, a1 = _rand((N, C2, H, W), gen), _rand((N, C1, H, W), gen).clamp(min=0)
    op = ConvOp(rt, w2.cuda(), None, [(C1, C1)], 1, 1, False, True)
    op.pack(H, W)
    dyv, a1v = View.alloc(rt, N, H, W, op.Cop), View.alloc(rt, N, H, W, C1)
    dyv.dense().copy_(_nhwc(dy, rt))
    a1v.dense().copy_(_nhwc(a1, rt))
    dz = View.alloc(rt, N, H, W, C1)
    dz.t.fill_(3.0)
    sums = rt.zeros((16, 2, C1), torch.float64)
    torch.cuda.synchronize()
    with knobs(fprop_dma_epi=epi, call_census=1):
        assert op.dgrad_actmask_ok(dyv, dz)
        nv.census_read()
        op.dgrad(dyv, dz, bn_reduce=(a1v, None, sums, act, 0.01))
        census = nv.census_read()
    torch.cuda.synchronize()
    return (w2, dy, a1), dz.dense().contiguous().cpu(), sums.cpu(), census


def test_epi_activation_mask_data_gradient():
    name = 'mask 16x16 64->64'
    (w2, dy, a1), dz1, s1, c1 = _launch_mask(1)
    _, dz1b, s1b, _ = _launch_mask(1)
    _, dz0, s0, c0 = _launch_mask(0)
    assert c1.get('epi:1') == 1 and c1.get('segnb_conv_fprop_bnreduce') == 1, c1
    assert 'epi:1' not in c0, c0
    msgs = []
    for what, a, ref, ref2 in (('dz', dz1, dz0, dz1b), ('bias-gradient sums (16 replicas)', s1, s0, s1b)):
        _same(name, msgs, what, a, ref, 'the plain order')
        _same(name, msgs, what, a, ref2, 'its own second launch')
    # float64: dx of the convolution, zero where the activated value is not positive (ReLU)
    r = eb.conv_refs(torch.zeros(dy.shape[0], w2.shape[1], dy.shape[2], dy.shape[3]), w2, None, dy, 1, 1, False)
    keep = (a1 > 0).double()
    worst, m = eb.within_bound(name + ' dz', dz1.float().permute(0, 3, 1, 2), r['dx'] * keep, r['mag_dx'] * keep, r['K_dx'], 'bf16')
    print('%s: dz worst err / bound %.3f' % (name, worst))
    msgs.append(m)
    tot = dz1.double().sum((0, 1, 2))
    rel = float(((s1.sum(0)[0] - tot).abs() / dz1.double().abs().sum((0, 1, 2))).max())
    print('%s: sums, worst |diff| / sum|dz| %.3g' % (name, rel))
    if not rel <= STAT_RTOL:
        msgs.append('%s: the sums differ from the stored dz by %.3g relative' % (name, rel))
    if float(s1[:, 1].abs().max()) != 0.0:
        msgs.append('%s: slot 1 of the sums is not zero' % name)
    msgs = [m for m in msgs if m]
    assert not msgs, '\n'.join(msgs)


# ------------------------------------------------------------------------------------------------ 2 x 2-window plane gather
# The data gradient of an up segment (UpCatConvOp.up).  Its store rows are chosen per step at run time (one or two a step), and
# that is the tap body's run-time mode (fprop_dma.hip: tap, ROW_RT), so the 2 x 2-window forms have no WsEpi
# instantiation: under knob 1 they keep the plain order and their bits.
# (N, S high resolution, Cu, Cs, Co, store rows per step or None where the gate declines the gather, so the general kernel runs it)
UPD = {
    '16->32 64+64->64': (2, 32, 64, 64, 64, 1),        # 4 chunks of 4 taps: one store row per step
    '16->32 64+64->32': (2, 32, 64, 64, 32, 2),        # 32-channel planes, 2 chunks: 7 steps carry 8 rows, two per step
    # 128 and 256 channels at 8 x 8 -> 16 x 16; below 12 low-resolution columns the plane gather is declined (fprop_dma.hip: upd_geometry)
    '8->16 128+128->128': (2, 16, 128, 128, 128, None),
    '8->16 256+256->256': (2, 16, 256, 256, 256, None),
}


@functools.lru_cache(maxsize=None)
def _upd_case(name):
    N, S, Cu, Cs, Co, _ = UPD[name]
    gen = torch.Generator().manual_seed(eb.seed_of('epi upd ' + name))
    w = torch.randn(Co, Cu + Cs, 3, 3, generator=gen) * (2.0 / ((Cu + Cs) * 9)) ** 0.5
    dy = _rand((N, Co, S, S), gen)
    wt = fe.phase_weights(w[:, :Cu])
    us = torch.zeros(N, Cu, S // 2, S // 2, dtype=torch.float64, requires_grad=True)
    F.conv_transpose2d(us, wt, None, stride=2, padding=1).backward(dy.double())
    return w, dy, us.grad, fe._du_mag(dy.double(), wt)


def _launch_upd(name, epi):
    N, S, Cu, Cs, Co, _ = UPD[name]
    w, dy, _, _ = _upd_case(name)
    rt = Runtime('cuda', 'bf16')
    op = UpCatConvOp(rt, w.cuda(), None, [(Cu, Cu), (Cs, Cs)], need_dgrad=True)
    PackTable(rt, op.up.pack_jobs(S // 2, S // 2), 'segnb_pack_weight_multi', 'segnb_pack_weight').run()
    dyv = View.alloc(rt, N, S, S, op.Cop)
    dyv.dense()[..., :Co] = _nhwc(dy, rt)
    duv = View.alloc(rt, N, S // 2, S // 2, Cu)
    duv.t.fill_(7.0)
    torch.cuda.synchronize()
    with knobs(fprop_dma_epi=epi, call_census=1):
        nv.census_read()
        op.up.dgrad(dyv, duv)
        census = nv.census_read()
    torch.cuda.synchronize()
    return duv.dense().contiguous().cpu(), census


@pytest.mark.parametrize('name', sorted(UPD))
def test_epi_up_segment_data_gradient(name):
    N, S, Cu, Cs, Co, rps = UPD[name]
    _, _, du_ref, du_mag = _upd_case(name)
    du1, c1 = _launch_upd(name, 1)
    du1b, _ = _launch_upd(name, 1)
    du0, c0 = _launch_upd(name, 0)
    assert 'epi:1' not in c1 and 'epi:1' not in c0, (c1, c0)
    assert c1 == c0 and c1.get('kernel:fprop_dma', 0) == (1 if rps is not None else 0), (c1, c0)
    msgs = []
    _same(name, msgs, 'du', du1, du0, 'the plain order')
    _same(name, msgs, 'du', du1, du1b, 'its own second launch')
    worst, m = eb.within_bound(name + ' du', du1.float().permute(0, 3, 1, 2), du_ref, du_mag, Co * 16, 'bf16')
    print('%s: du worst err / bound %.3f' % (name, worst))
    msgs.append(m)
    msgs = [m for m in msgs if m]
    assert not msgs, '\n'.join(msgs)


# ------------------------------------------------------------------------------------------------ kept on the plain order
@pytest.mark.parametrize('name,shape,ksplit', [('tall 7x7 128->72', (5, 7, 7, 128, 72), 0), ('split K 7x7 256->72', (5, 7, 7, 256, 72), 2)])
def test_epi_knob_leaves_tall_and_split_k_alone(name, shape, ksplit):
    """the tall 7 x 7 form (32x32x16 stream) and its split-K launches have no WsEpi instantiation: under knob 1 they run the plain
    order -- no "epi:1" in the census, the bits of knob 0, and the derived bound holds"""
    N, H, W, Ci, Co = shape
    w, b, x, dy, r = _plain_case(name, N, H, W, Ci, Co)
    y1, st1, dx1, c1 = _launch_plain(w, b, x, dy, 1, ksplit=ksplit)
    y0, st0, dx0, c0 = _launch_plain(w, b, x, dy, 0, ksplit=ksplit)
    assert 'epi:1' not in c1 and c1.get('kernel:fprop_dma', 0) >= 1, c1
    assert c1 == c0, (c1, c0)
    msgs = []
    _same(name, msgs, 'y', y1, y0, 'knob 0')
    _same(name, msgs, 'dx', dx1, dx0, 'knob 0')
    if ksplit == 0:             # (the slabs of a split launch are added by whichever block comes last, in slice order: same sums too)
        _same(name, msgs, 'statistics', st1, st0, 'knob 0')
    _check_bounds(name, msgs, y1, dx1, r, Ci, Co)
    _check_stats(name, msgs, st1, y1, Co)
    msgs = [m for m in msgs if m]
    assert not msgs, '\n'.join(msgs)
