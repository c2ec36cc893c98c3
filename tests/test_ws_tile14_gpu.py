"""-m gpu: the 14 x 14-pixel tile of conv_fprop_ws_kernel (224 matrix rows, segnb_tune "fprop_dma_cfg" = 3) against its 16 x 16
tile (cfg 1) and against float64.

Every geometry runs under cfg 3 first -- fresh tensors, the first launch of that geometry in the test: a counted wait that misses
a fetch shows on a cold launch only -- then under cfg 3 again, then under cfg 1:

  * the stored outputs (y, dx) of cfg 3 are the bits of cfg 1 (the per-element K order is the same), and of its own second run;
  * they lie within the derived bound of tests/errbound.py around F.conv2d in float64 on the CPU;
  * the forward's statistics, summed over the 16 replicas, are the float64 sum and sum of squares of the STORED y to 1e-6
    relative (operands with a bias of about one, so that the sums are well conditioned);
  * at 14 x 14, where both tilings hold one image per tile, the statistics of cfg 3 are those of cfg 1 bit for bit (the store pass
    keeps the 16 x 16 tile's pixel -> thread assignment), so a training step's outputs do not move;
  * the launches were served by the 14 x 14 tile (the call census counts "tile:ws14" beside "kernel:fprop_dma").

Geometries the gate of dispatch_fd refuses (15 x 15; a data gradient with an activation mask) keep their present tile when cfg 3
is forced: no "tile:ws14" in the census, and their present checks hold."""
import functools

import pytest
import torch
import torch.nn.functional as F

import errbound as eb
from segnb import _native as nv
from segnb import convplan as cp
from segnb.engine import ConvOp, PackTable, Runtime, UpCatConvOp, View

pytestmark = pytest.mark.gpu

# name: (N, H, W, Ci, Co, conv_cu_pct or None)
PLAIN = {
    '14x14 64->64': (2, 14, 14, 64, 64, None),         # one tile per image, one chunk
    '14x14 128->192': (3, 14, 14, 128, 192, None),     # two chunks, three channel tiles; the default selection's 14 x 14 case
    '28x28 128->64': (2, 28, 28, 128, 64, None),       # four tiles, two chunks: the halo double buffer crosses tiles
    '28x28 64->192': (2, 28, 28, 64, 192, None),       # three channel tiles: the last block's tile stream
    # 16 tiles on 2 % of the CUs (5 of 256: the knob is a percentage): 4, 3, 3, 3, 3 tiles per persistent block
    '56x56 64->64': (1, 56, 56, 64, 64, 2),
}
STAT_RTOL = 1e-6


class knobs(object):
    """segnb_tune settings for a block, back at their defaults afterwards"""
    DEFAULTS = {'fprop_dma_cfg': -1, 'conv_cu_pct': 100, 'call_census': 0}

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


@functools.lru_cache(maxsize=None)
def _plain_case(name, N, H, W, Ci, Co):
    """operands (bf16-exact) and the float64 references of a 3 x 3 / pad 1 convolution, computed once per geometry"""
    gen = torch.Generator().manual_seed(eb.seed_of(name))
    w = _rand((Co, Ci, 3, 3), gen, (2.0 / (Ci * 9)) ** 0.5)
    b = 1.0 + 0.1 * torch.randn(Co, generator=gen)
    x, dy = _rand((N, Ci, H, W), gen), _rand((N, Co, H, W), gen)
    return w, b, x, dy, eb.conv_refs(x, w, b, dy, 1, 1, False)


def _launch_plain(w, b, x, dy, cfg, cu_pct=None):
    """forward with statistics and data gradient on FRESH tensors under fprop_dma_cfg = cfg
    -> raw bf16 y [N,H,W,Co], statistics [2,Co] (replicas summed), raw bf16 dx, census of the two launches"""
    N, Ci, H, W = x.shape
    Co = w.shape[0]
    rt = Runtime('cuda', 'bf16')
    op = ConvOp(rt, w.cuda(), b.cuda(), [(Ci, Ci)], 1, 1, False, need_dgrad=True)
    op.pack(H, W)
    xv, dyv = View.alloc(rt, N, H, W, Ci), View.alloc(rt, N, H, W, Co)
    xv.dense().copy_(_nhwc(x, rt))
    dyv.dense().copy_(_nhwc(dy, rt))
    yv, dxv = View.alloc(rt, N, H, W, Co), View.alloc(rt, N, H, W, Ci)
    yv.t.fill_(3.0)
    dxv.t.fill_(3.0)
    stats = rt.zeros((16, 2, Co), torch.float64)
    torch.cuda.synchronize()
    with knobs(fprop_dma_cfg=cfg, conv_cu_pct=cu_pct, call_census=1):
        nv.census_read()
        op.fprop(xv, yv, stats)
        op.dgrad(dyv, dxv)
        census = nv.census_read()
    torch.cuda.synchronize()
    return yv.dense().contiguous().cpu(), stats.sum(0).cpu(), dxv.dense().contiguous().cpu(), census


def _check_stats(name, msgs, st, y_raw):
    v = y_raw.double().reshape(-1, y_raw.shape[-1])
    for row, what, tot in ((0, 'sum', v.sum(0)), (1, 'sum of squares', (v * v).sum(0))):
        rel = ((st[row] - tot).abs() / tot.abs()).max()
        print('%s: statistics %s, worst relative difference from the float64 sum of the stored y %.3g' % (name, what, float(rel)))
        if not bool(rel <= STAT_RTOL):
            msgs.append('%s: %s of the epilogue differs from the stored y by %.3g relative (> %g)' % (name, what, float(rel), STAT_RTOL))


def _check_bounds(name, msgs, y_raw, dx_raw, r):
    for what, got, ref, mag, K in (('y', y_raw, r['y'], r['mag_y'], r['K_y']), ('dx', dx_raw, r['dx'], r['mag_dx'], r['K_dx'])):
        worst, m = eb.within_bound('%s %s' % (name, what), got.float().permute(0, 3, 1, 2), ref, mag, K, 'bf16')
        print('%s: %s worst err / bound %.3f' % (name, what, worst))
        msgs.append(m)


@pytest.mark.parametrize('name', sorted(PLAIN))
def test_tile14_forward_and_data_gradient(name):
    N, H, W, Ci, Co, cu_pct = PLAIN[name]
    w, b, x, dy, r = _plain_case(name, N, H, W, Ci, Co)
    y3, st3, dx3, c3 = _launch_plain(w, b, x, dy, 3, cu_pct)          # cold: the first launches of this geometry, fresh tensors
    y3b, st3b, dx3b, _ = _launch_plain(w, b, x, dy, 3, cu_pct)
    y1, st1, dx1, c1 = _launch_plain(w, b, x, dy, 1, cu_pct)
    assert c3.get('tile:ws14') == 2 and c3.get('kernel:fprop_dma') == 2, c3
    assert 'tile:ws14' not in c1 and c1.get('kernel:fprop_dma') == 2, c1
    msgs = []
    for what, a, ref in (('y', y3, y1), ('dx', dx3, dx1)):
        if not torch.equal(a.view(torch.int16), ref.view(torch.int16)):
            bad = (a.view(torch.int16) != ref.view(torch.int16))
            msgs.append('%s: %s of the 14 x 14 tile differs from the 16 x 16 tile in %d/%d elements, first %s' % (
                name, what, int(bad.sum()), bad.numel(), bad.nonzero()[:4].tolist()))
    for what, a, ref in (('y', y3, y3b), ('dx', dx3, dx3b), ('statistics', st3, st3b)):
        same = torch.equal(a.view(torch.int16), ref.view(torch.int16)) if a.dtype == torch.bfloat16 else torch.equal(a, ref)
        if not same:
            msgs.append('%s: %s differs between the cold launch and the second one' % (name, what))
    if H == 14 and not torch.equal(st3, st1):
        msgs.append('%s: the statistics of the 14 x 14 tile are not the bits of the 16 x 16 tile (worst difference %.3g)' % (
            name, float((st3 - st1).abs().max())))
    _check_bounds(name, msgs, y3, dx3, r)
    _check_stats(name + ' cfg 3', msgs, st3, y3)
    _check_stats(name + ' cfg 1', msgs, st1, y1)
    msgs = [m for m in msgs if m]
    assert not msgs, '\n'.join(msgs)


@pytest.mark.parametrize('name,served', [('14x14 128->192', 2), ('28x28 64->192', 1)])
def test_tile14_default_selection_keeps_every_bit(name, served):
    """fprop_dma_cfg = -1: dispatch_fd picks the tile on its own (rounds x rows: 224 < 256) for the data gradients of the
    measured levels and, where the statistics stay bit for bit (14 x 14), for the forwards: forward + data gradient are served
    by it twice at 14 x 14, once at 28 x 28 -- and y, dx AND the statistics are those of the 16 x 16 tile"""
    N, H, W, Ci, Co, _ = PLAIN[name]
    w, b, x, dy, r = _plain_case(name, N, H, W, Ci, Co)
    y0, st0, dx0, c0 = _launch_plain(w, b, x, dy, -1)
    y1, st1, dx1, c1 = _launch_plain(w, b, x, dy, 1)
    assert c0.get('tile:ws14') == served and c0.get('kernel:fprop_dma') == 2, c0
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16)) and torch.equal(dx0.view(torch.int16), dx1.view(torch.int16))
    assert torch.equal(st0, st1), float((st0 - st1).abs().max())


# ------------------------------------------------------------------------------------------------ virtual concat
@functools.lru_cache(maxsize=None)
def _upcat_case():
    """28 x 28, (64 upsampled + 64 skip) -> 64: operands and float64 references over the materialised concat"""
    N, S, Cu, Cs, Co = 2, 28, 64, 64, 64
    gen = torch.Generator().manual_seed(eb.seed_of('upcat 28x28 64+64->64'))
    w = _rand((Co, Cu + Cs, 3, 3), gen, (2.0 / ((Cu + Cs) * 9)) ** 0.5)
    b = 1.0 + 0.1 * torch.randn(Co, generator=gen)
    u, sk, dy = _rand((N, Cu, S // 2, S // 2), gen), _rand((N, Cs, S, S), gen), _rand((N, Co, S, S), gen)
    cat = torch.cat([F.interpolate(u, scale_factor=2, mode='nearest'), sk], 1)
    return (N, S, Cu, Cs, Co), w, b, u, sk, dy, eb.conv_refs(cat, w, b, dy, 1, 1, False)


def _launch_upcat(cfg):
    """virtual-concat forward (statistics) and the skip segment's data gradient into its slice of the concat gradient, fresh
    tensors -> raw y, statistics [2,Co], raw gradient buffer [N,S,S,Cu+Cs], census"""
    (N, S, Cu, Cs, Co), w, b, u, sk, dy, _ = _upcat_case()
    rt = Runtime('cuda', 'bf16')
    op = UpCatConvOp(rt, w.cuda(), b.cuda(), [(Cu, Cu), (Cs, Cs)], need_dgrad=True)
    op.virtual_concat = True
    PackTable(rt, op.full.pack_jobs(S, S) + op.skip.pack_jobs(S, S), 'segnb_pack_weight_multi', 'segnb_pack_weight').run()
    cat = View.alloc(rt, N, S, S, Cu + Cs)
    cat.t.fill_(5.0)                                     # the upsampled copy is not read: left as garbage
    cat.dense()[..., Cu:] = _nhwc(sk, rt)
    uv, duv = View.alloc(rt, N, S // 2, S // 2, Cu), View.alloc(rt, N, S // 2, S // 2, Cu)
    uv.dense().copy_(_nhwc(u, rt))
    op.bind_up(uv, duv)
    assert op.virtual(N, S, S), 'the virtual concat does not serve 28 x 28, 64 + 64 -> 64'
    dyv = View.alloc(rt, N, S, S, Co)
    dyv.dense().copy_(_nhwc(dy, rt))
    yv, dcat = View.alloc(rt, N, S, S, Co), View.alloc(rt, N, S, S, Cu + Cs)
    yv.t.fill_(3.0)
    dcat.t.fill_(7.0)
    stats = rt.zeros((16, 2, Co), torch.float64)
    torch.cuda.synchronize()
    with knobs(fprop_dma_cfg=cfg, call_census=1):
        nv.census_read()
        op.fprop(cat, yv, stats)
        op.skip.dgrad(dyv, dcat.slice(Cu, Cs))
        census = nv.census_read()
    torch.cuda.synchronize()
    return yv.dense().contiguous().cpu(), stats.sum(0).cpu(), dcat.dense().contiguous().cpu(), census


def test_tile14_virtual_concat_forward_and_skip_data_gradient():
    (N, S, Cu, Cs, Co), w, b, u, sk, dy, r = _upcat_case()
    name = 'upcat 28x28 64+64->64'
    y3, st3, d3, c3 = _launch_upcat(3)
    y3b, st3b, d3b, _ = _launch_upcat(3)
    y1, st1, d1, c1 = _launch_upcat(1)
    assert c3.get('tile:ws14') == 2 and 'tile:ws14' not in c1, (c3, c1)
    msgs = []
    if not torch.equal(y3.view(torch.int16), y1.view(torch.int16)):
        msgs.append('y of the 14 x 14 tile differs from the 16 x 16 tile')
    if not torch.equal(d3.view(torch.int16), d1.view(torch.int16)):
        msgs.append('skip-segment dx of the 14 x 14 tile differs from the 16 x 16 tile')
    if not (torch.equal(y3.view(torch.int16), y3b.view(torch.int16)) and torch.equal(d3.view(torch.int16), d3b.view(torch.int16))
            and torch.equal(st3, st3b)):
        msgs.append('the cold launch and the second one differ')
    if float((d3[..., :Cu].float() - 7.0).abs().max()) != 0.0:
        msgs.append('the skip segment\'s data gradient wrote outside its channel slice')
    worst, m = eb.within_bound(name + ' y', y3.float().permute(0, 3, 1, 2), r['y'], r['mag_y'], r['K_y'], 'bf16')
    msgs.append(m)
    worst, m = eb.within_bound(name + ' skip dx', d3[..., Cu:].float().permute(0, 3, 1, 2), r['dx'][:, Cu:], r['mag_dx'][:, Cu:],
                               r['K_dx'], 'bf16')
    msgs.append(m)
    _check_stats(name + ' cfg 3', msgs, st3, y3)
    msgs = [m for m in msgs if m]
    assert not msgs, '\n'.join(msgs)


# ------------------------------------------------------------------------------------------------ declined, not mis-served
def test_tile14_declines_15x15():
    """15 x 15 is not made of 14 x 14 tiles: forced cfg 3 takes the tile dispatch_fd chooses on its own (16 x 16)"""
    name = '15x15 64->64'
    w, b, x, dy, r = _plain_case(name, 2, 15, 15, 64, 64)
    y3, st3, dx3, c3 = _launch_plain(w, b, x, dy, 3)
    y0, st0, dx0, c0 = _launch_plain(w, b, x, dy, 1)
    assert 'tile:ws14' not in c3 and c3.get('kernel:fprop_dma') == 2, c3
    assert c0 == c3, (c0, c3)
    assert torch.equal(y3.view(torch.int16), y0.view(torch.int16)) and torch.equal(dx3.view(torch.int16), dx0.view(torch.int16))
    assert torch.equal(st3, st0)
    msgs = []
    _check_bounds(name, msgs, y3, dx3, r)
    _check_stats(name, msgs, st3, y3)
    msgs = [m for m in msgs if m]
    assert not msgs, '\n'.join(msgs)


def test_tile14_declines_activation_mask():
    """28 x 28 with the producing layer's activation mask on the data gradient (bn_y set): the MASK instantiation lives on the
    16 x 16 tile, forced cfg 3 leaves it there -- dz == segnb_bn_act_bwd_reduce(plain dx, activated tensor) bit for bit and the
    bias-gradient sums agree, as in test_hip_ops.test_conv_dgrad_with_act_mask"""
    N, H, W, C1, C2, act = 2, 28, 28, 64, 64, nv.ACT_RELU
    rt = Runtime('cuda', 'bf16')
    gen = torch.Generator().manual_seed(2814)
    w2 = _rand((C2, C1, 3, 3), gen, (2.0 / (C1 * 9)) ** 0.5).cuda()
    op = ConvOp(rt, w2, None, [(C1, cp.pad8(C1))], 1, 1, False, True)
    op.pack(H, W)
    dyv, a1 = View.alloc(rt, N, H, W, op.Cop), View.alloc(rt, N, H, W, C1)
    dyv.dense().copy_(_nhwc(_rand((N, C2, H, W), gen), rt))
    a1.dense().copy_(_nhwc(_rand((N, C1, H, W), gen).clamp(min=0), rt))
    dx_plain, dz_ref, dz_f = (View.alloc(rt, N, H, W, C1) for _ in range(3))
    sums_ref, sums_f = rt.zeros((16, 2, C1), torch.float64), rt.zeros((16, 2, C1), torch.float64)
    st = torch.cuda.current_stream().cuda_stream
    with knobs(fprop_dma_cfg=3, call_census=1):
        nv.census_read()
        op.dgrad(dyv, dx_plain)
        c_plain = nv.census_read()
        nv.call('segnb_bn_act_bwd_reduce', rt.code, a1.ptr, a1.ld, N, H, W, C1, None, act, 0.01, None, dx_plain.ptr, dx_plain.ld,
                None, 0, None, 0, dz_ref.ptr, dz_ref.ld, nv.ptr(sums_ref), None, 0, st)
        assert op.dgrad_actmask_ok(dyv, dx_plain)
        nv.census_read()
        op.dgrad(dyv, dz_f, bn_reduce=(a1, None, sums_f, act, 0.01))
        c_mask = nv.census_read()
    torch.cuda.synchronize()
    assert c_plain.get('tile:ws14') == 1, c_plain
    assert 'tile:ws14' not in c_mask and c_mask.get('segnb_conv_fprop_bnreduce') == 1, c_mask
    assert torch.equal(dz_f.t, dz_ref.t)
    a, b = sums_f.sum(0).cpu(), sums_ref.sum(0).cpu()
    assert float(a[1].abs().max()) == 0.0
    assert float((a[0] - b[0]).abs().max()) <= 2e-5 * float(b[0].abs().max()) + 1e-6 * (N * H * W) ** 0.5
