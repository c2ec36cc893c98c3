"""CPU-only checks of dilated convolutions in the convolution plan (segnb.convplan, ConvOp, conv_unit):

  * segnb.convplan with dilation 1, 2, 4: forward and data-gradient tap tables applied through the emulator's gather against
    float64 F.conv2d(dilation) and its autograd; dilation 1 reproduces the tables of the plan without the argument;
  * every fused `*_ok` predicate of the library (host code) refuses a dilated table at shapes inside its own size gates;
  * conv_unit(dilation=d) with BatchNorm, residual and ReLU, eval and training, forward and backward, through the ABI on the
    emulator against float64 (tests/dilated_net.py); ConvOp with a stride != 1 or transposed and a dilation raises.
"""
import os

import pytest
import torch
import torch.nn.functional as F

from oracle.abi_emulator import AbiEmulator, _gather
from segnb import _native as nv
from segnb import convplan as cp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- dilation in the convolution plan --------------------------------------------------------------------------------------------
def _geom(launch, N, Hi, Wi, Ci, Ho, Wo, Co):
    from segnb.engine import ConvOp
    return ConvOp._make_geom(launch, N, Hi, Wi, Ci, Ci, Ho, Wo, Co, Co)


def _apply(launches, src, w_of_tap, N, Hs, Ws, Cs, Hd, Wd, Cd):
    """run tap-table launches the way segnb_conv_fprop does (oracle.abi_emulator._gather): src [N, Hs, Ws, Cs] -> [N, Hd, Wd, Cd];
    w_of_tap(kh, kw) -> the [Cd, Cs] matrix of one tap"""
    out = torch.zeros(N, Hd, Wd, Cd, dtype=torch.float64)
    for l in launches:
        g = _geom(l, N, Hs, Ws, Cs, Hd, Wd, Cd)
        acc = torch.zeros(N, l.QH, l.QW, Cd, dtype=torch.float64)
        for t, (_, _, a, b) in enumerate(l.taps):
            acc += _gather(src, g, t).double() @ w_of_tap(a, b).t()
        out[:, l.oh0::l.out_step, l.ow0::l.out_step][:, :l.QH, :l.QW] = acc
    return out


@pytest.mark.parametrize('d', [1, 2, 4])
@pytest.mark.parametrize('k,pad', [(3, None), (3, 0), (1, 0)])
def test_convplan_dilation_against_conv2d(d, k, pad):
    pad = d * (k // 2) if pad is None else pad
    N, H, W, Ci, Co = 2, 11, 13, 8, 16
    gen = torch.Generator().manual_seed(100 * d + k)
    x = torch.randn(N, Ci, H, W, generator=gen).double().requires_grad_(True)          # (fp32-exact: the gather returns fp32)
    w = torch.randn(Co, Ci, k, k, generator=gen).double()
    y = F.conv2d(x, w, None, stride=1, padding=pad, dilation=d)
    (Ho, Wo), fwd = cp.conv_fwd(H, W, k, k, 1, pad, d)
    assert (Ho, Wo) == tuple(y.shape[2:]) == (cp.conv_out_size(H, k, 1, pad, d), cp.conv_out_size(W, k, 1, pad, d))
    got = _apply(fwd, x.detach().permute(0, 2, 3, 1), lambda a, b: w[:, :, a, b], N, H, W, Ci, Ho, Wo, Co)
    assert float((got - y.detach().permute(0, 2, 3, 1)).abs().max()) < 1e-12
    gy = torch.randn(y.shape, generator=gen).double()
    y.backward(gy)
    dg, full = cp.conv_dgrad(H, W, k, k, 1, pad, d)
    assert full and len(dg) == 1
    gx = _apply(dg, gy.permute(0, 2, 3, 1), lambda a, b: w[:, :, a, b].t(), N, Ho, Wo, Co, H, W, Ci)
    assert float((gx - x.grad.permute(0, 2, 3, 1)).abs().max()) < 1e-12
    # a dilated 3 x 3 keeps 9 taps whose offsets span 2 * d: what the fast paths' gate (csrc/common.h: segnb_taps_3x3) refuses
    if k == 3:
        for l in fwd + dg:
            assert len(l.taps) == 9
            assert max(t[0] for t in l.taps) - min(t[0] for t in l.taps) == 2 * d
            assert max(t[1] for t in l.taps) - min(t[1] for t in l.taps) == 2 * d


@pytest.mark.parametrize('k,stride,pad', [(3, 1, 1), (3, 1, 0), (3, 2, 1), (7, 2, 3), (1, 1, 0), (1, 2, 0), (2, 1, 1), (4, 2, 1)])
def test_convplan_dilation_1_is_the_plan_without_it(k, stride, pad):
    for H, W in ((16, 16), (9, 14)):
        assert cp.conv_fwd(H, W, k, k, stride, pad, 1) == cp.conv_fwd(H, W, k, k, stride, pad)
        assert cp.conv_dgrad(H, W, k, k, stride, pad, 1) == cp.conv_dgrad(H, W, k, k, stride, pad)
        assert cp.conv_out_size(H, k, stride, pad, 1) == (H + 2 * pad - k) // stride + 1
    # today's dense 3 x 3 tables, spelled out
    (Ho, Wo), (l,) = cp.conv_fwd(8, 8, 3, 3, 1, 1)
    assert (Ho, Wo) == (8, 8) and l.taps == [(a - 1, b - 1, a, b) for a in range(3) for b in range(3)]
    (l,), full = cp.conv_dgrad(8, 8, 3, 3, 1, 1)
    assert full and l.taps == [(1 - a, 1 - b, a, b) for a in range(3) for b in range(3)]


@pytest.fixture
def emulated():
    nv.set_backend_for_testing(AbiEmulator())
    yield
    nv.set_backend_for_testing(None)


def test_dilated_conv_units_on_the_emulator(emulated):
    """conv_unit(dilation=d) -> BatchNorm -> (+ residual) -> ReLU, three layers deep (tests/dilated_net.py), through the ABI on
    the emulator: eval forward, then a training step in the same tape, against the float64 torch function.  fp32 sums of at most
    576 products per layer, three layers: 1e-4 of the logit scale and 1e-3 relative L2 per gradient tensor leave two orders of
    magnitude over the rounding error (6e-8 * sqrt(576) per layer)."""
    import dilated_net as DN
    torch.manual_seed(2)
    m = DN.DilatedNet(num_classes=2).set_compute_dtype('f32')
    gen = torch.Generator().manual_seed(3)
    x, G = torch.randn(2, 3, 12, 20, generator=gen), torch.randn(2, 2, 12, 20, generator=gen)
    ev, out, grads, bufs = DN.reference_step(m, x, G)
    m.eval()
    with torch.no_grad():
        got = m(x)
    assert float((got.double() - ev).abs().max()) <= 1e-4 * float(ev.abs().max())
    m.train()
    got = m(x)
    (got * G).sum().backward()
    assert float((got.detach().double() - out).abs().max()) <= 1e-4 * float(out.abs().max())
    for n, p in m.named_parameters():
        rel = float((p.grad.double() - grads[n]).norm() / (grads[n].norm() + 1e-30))
        assert rel <= 1e-3, (n, rel)
    for k, b in m.named_buffers():
        if 'num_batches' not in k:
            assert float((b.double() - bufs[k]).abs().max()) <= 1e-5, k
    # every plan of the model carries the spread tables
    spans = sorted(max(t[0] for t in l.taps) - min(t[0] for t in l.taps)
                   for conv, h, w in m._tape.convs for l in conv.plan(h, w)['fwd'])
    assert spans == [4, 4, 8]


def test_fused_predicates_refuse_a_dilated_table():
    """every `*_ok` of the library (host predicates: no device needed) says no to a dilated 3 x 3 at shapes inside its own size
    gates -- forward and flipped table, d = 2 and 4 -- including both arms of segnb_conv_fprop_drop_ok"""
    if not os.path.exists(nv.LIB_PATH):
        pytest.skip('libsegnb_hip.so not built (run __graft_entry__.build())')
    from segnb.engine import ConvOp

    def geom(launch, N, H, W, Ci, Co):
        return ConvOp._make_geom(launch, N, H, W, Ci, Ci, H, W, Co, Co)
    for d in (2, 4):
        (_, _), (fwd,) = cp.conv_fwd(32, 32, 3, 3, 1, d, d)
        (dg,), _ = cp.conv_dgrad(32, 32, 3, 3, 1, d, d)
        for l in (fwd, dg):
            thin = geom(l, 2, 32, 32, 32, 32)                 # rolling / tf / actmask / bnreduce sizes
            for name, g, extra in [('segnb_conv_fprop_bnreduce_ok', thin, ()), ('segnb_conv_fprop_bnreduce_ok', geom(l, 2, 32, 32, 16, 64), ()),
                                   ('segnb_conv_fprop_bnapply_ok', geom(l, 2, 32, 32, 16, 64), ()),
                                   ('segnb_conv_fprop_actmask_ok', thin, ()), ('segnb_conv_fprop_actmask_ok', geom(l, 2, 32, 32, 64, 64), ()),
                                   ('segnb_conv_fprop_tf_ok', thin, (nv.TF_ACT,)), ('segnb_conv_fprop_tf_ok', thin, (nv.TF_BNBWD,)),
                                   ('segnb_conv_wgrad_tf_ok', thin, ()), ('segnb_conv_wgrad_bnapply_ok', geom(l, 2, 32, 32, 8, 32), ()),
                                   ('segnb_conv_fprop_drop_ok', geom(l, 2, 32, 32, 128, 16), ()),      # the stride-1 3 x 3 arm
                                   ('segnb_conv_fprop_drop_ok', geom(l, 1, 8, 8, 1024, 16), ()),       # the deep-K arm
                                   ('segnb_conv_fprop_u8_ok', geom(l, 2, 32, 32, 8, 32), ()),
                                   ('segnb_conv_fprop_upd_ok', thin, ()),
                                   ('segnb_conv_upcat_ok', geom(l, 2, 32, 32, 64, 32), (32,)),
                                   ('segnb_conv_fprop_upsum_ok', geom(l, 2, 32, 32, 32, 32), (32,))]:
                assert nv.query(name, g, nv.BF16, *extra) == 0, (name, d)
            assert nv.query('segnb_conv_wgrad_slabs', thin, nv.BF16) == 1          # (no fast-path slabs: the general kernel)


def test_convop_dilation_arguments():
    from segnb.engine import ConvOp, Runtime
    rt = Runtime('cpu', 'f32')
    w = torch.zeros(16, 8, 3, 3)
    op = ConvOp(rt, w, None, [(8, 8)], stride=1, pad=2, dilation=2)
    assert op.dilation == 2 and op._taps(cp.conv_fwd(8, 8, 3, 3, 1, 2, 2)[1][0]) == list(range(9))      # packed tap -> a * KW + b
    assert ConvOp(rt, w, None, [(8, 8)]).dilation == 1
    with pytest.raises(ValueError, match='dilation'):
        ConvOp(rt, w, None, [(8, 8)], stride=2, pad=2, dilation=2)
    with pytest.raises(ValueError, match='dilation'):
        ConvOp(rt, w, None, [(16, 16)], stride=1, pad=2, transposed=True, dilation=2)
    with pytest.raises(ValueError, match='dilation'):
        ConvOp(rt, w, None, [(8, 8)], dilation=0)
