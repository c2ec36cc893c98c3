"""Dilated convolutions on the MI355X:

  1. dilated ConvOp forward (with the fused BatchNorm statistics), data gradient and weight gradient against float64
     F.conv2d(dilation) autograd on the dtype-rounded operands, element by element under errbound.bound_of; every launch of a
     dilated op is served by a kernel that walks the tap table (the census names it).  The dense d = 1 control on the same
     operands must be served by the kernels this build's selectors choose for it (DENSE_BF16: read off the gates; the parent
     commit has no kernel census to compare with).  Only the 64 -> 64 and 32 -> 64 shapes reach a specialised kernel when dense
     (fprop_dma, fprop_rw, wgrad_s1); the two 8 x 8 shapes go to the general / deep-K kernels either way, so the guards of
     fprop_roll, fprop_thin, fprop_c8, fprop_s1, wgrad_roll and wgrad_c8roll are verified by reading, by the predicate test of
     tests/test_dilation_cpu.py, and by 2 below;
  2. conv_unit(dilation) through the tape (tests/dilated_net.py): eval, then eager / recorded / replayed training steps against
     float64, at shapes inside the size gates of the c8, rolling, resident-weight and LDS-DMA kernels and their fused BatchNorm
     forms; the census holds no fused entry point and only table-walking kernels.
"""
import pytest
import torch
import torch.nn.functional as F

import errbound as eb
from segnb import _native as nv
from segnb.engine import ConvOp, Runtime, View

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
F64 = torch.float64
DTYPES = ['f32', 'bf16']


def _st():
    return torch.cuda.current_stream(DEV).cuda_stream


def _tdt(dtype):
    return (nv.F32, torch.float32) if dtype == 'f32' else (nv.BF16, torch.bfloat16)


def _randn(shape, seed, dtype='f32', scale=1.0):
    """fp32 values on the CPU that are exact in `dtype`"""
    t = torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale
    return t.bfloat16().float() if dtype == 'bf16' else t


def _within(name, got, ref, mag, T, dtype):
    worst, msg = eb.within_bound(name, got.detach().float().cpu(), ref.detach(), mag.detach(), T, dtype)
    print('%s [%s]: worst err/bound %.3f' % (name, dtype, worst))
    assert msg is None, msg


# ------------------------------------------------------------------------------------------------- 1. dilated convolutions
DILATED = [(2, 16, 16, 64, 64, 2), (2, 12, 20, 32, 64, 4), (1, 8, 8, 256, 256, 2), (1, 8, 8, 512, 512, 4)]
TABLE_WALKERS = {'kernel:fprop_general', 'kernel:fprop_deepk'}       # forward kernels that read dh[] / dw[] for every tap
# the kernels that serve the dense 3 x 3 control in bf16 (forward with statistics, data gradient, weight gradient) by the selectors'
# own gates: 64 and 32 input channels at these widths go to the LDS-DMA / resident-weight pipelines, the 8 x 8 maps are too narrow
# for every 3 x 3 pipeline (the deep-K kernel takes their plain launch).  The span helper (csrc/common.h: segnb_taps_3x3) holds for
# every dense 3 x 3, so the helper cannot have changed them -- but they are this build's choices: the parent had no census
DENSE_BF16 = {(2, 16, 16, 64, 64): ('kernel:fprop_dma', 'kernel:fprop_dma', 'kernel:wgrad_s1'),
              (2, 12, 20, 32, 64): ('kernel:fprop_rw', 'kernel:fprop_rw', 'kernel:wgrad_general'),
              (1, 8, 8, 256, 256): ('kernel:fprop_general', 'kernel:fprop_deepk', 'kernel:wgrad_general'),
              (1, 8, 8, 512, 512): ('kernel:fprop_general', 'kernel:fprop_deepk', 'kernel:wgrad_general')}


class census(object):
    """the call census around a block -> .names: one {name: count} per nv.census_read() taken inside"""

    def __enter__(self):
        nv.call('segnb_tune', b'call_census', 1)
        nv.census_read()
        return self

    def take(self):
        return {k: v for k, v in nv.census_read().items() if k.startswith('kernel:')}

    def __exit__(self, *a):
        nv.call('segnb_tune', b'call_census', 0)


def _run_conv(dtype, N, H, W, Ci, Co, d, w, x, dy):
    """-> y [N,H,W,Co], sums [2,Co], dx [N,H,W,Ci], dW, the kernel names of the three launches"""
    rt = Runtime(DEV, dtype)
    wt = w.to(DEV)
    op = ConvOp(rt, wt, None, [(Ci, Ci)], 1, d, False, need_dgrad=True, dilation=d)
    op.pack(H, W)
    assert op.out_hw(H, W) == (H, W)
    ld = Ci + 8                                              # a view with ld != C, as the executor's slices have
    xv = View(rt.zeros((N, H, W, ld)), N, H, W, Ci, ld, 8)
    xv.dense().copy_(x.permute(0, 2, 3, 1).to(DEV, rt.tdtype))
    yv, dyv, dxv = View.alloc(rt, N, H, W, Co), View.alloc(rt, N, H, W, Co), View.alloc(rt, N, H, W, Ci)
    dyv.dense().copy_(dy.permute(0, 2, 3, 1).to(DEV, rt.tdtype))
    stats = rt.zeros((16, 2, Co), torch.float64)             # SEGNB_STAT_REPLICAS copies
    gw = torch.zeros_like(wt)
    with census() as c:
        op.fprop(xv, yv, stats)
        kf = c.take()
        op.dgrad(dyv, dxv)
        kd = c.take()
        op.wgrad(xv, dyv, gw)
        kw = c.take()
    torch.cuda.synchronize()
    for k in (kf, kd, kw):
        assert sum(k.values()) == 1, k
    return (yv.dense().float().cpu(), stats.sum(0).cpu(), dxv.dense().float().cpu(), gw.cpu(),
            tuple(list(k)[0] for k in (kf, kd, kw)))


def _refs(x, w, dy, d):
    def three(x, w, dy):
        x, w = x.double().requires_grad_(True), w.double().requires_grad_(True)
        y = F.conv2d(x, w, None, padding=d, dilation=d)
        y.backward(dy.double())
        return y.detach(), x.grad, w.grad
    return three(x, w, dy), three(x.abs(), w.abs(), dy.abs())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('N,H,W,Ci,Co,d', DILATED, ids=lambda v: str(v))
def test_dilated_conv_within_derived_bound(N, H, W, Ci, Co, d, dtype):
    w = _randn((Co, Ci, 3, 3), 31 + d, dtype, (2.0 / (Ci * 9)) ** 0.5)
    x, dy = _randn((N, Ci, H, W), 32 + d, dtype), _randn((N, Co, H, W), 33 + d, dtype)
    (y, dx, dW), (my, mdx, mdW) = _refs(x, w, dy, d)
    gy, st, gdx, gdW, names = _run_conv(dtype, N, H, W, Ci, Co, d, w, x, dy)
    print('dilation %d %s: served by %s' % (d, dtype, names))
    # every fast path declines a dilated table: the kernels that walk the tap table serve the three launches
    assert names[0] in TABLE_WALKERS and names[1] in TABLE_WALKERS and names[2] == 'kernel:wgrad_general', names
    _within('y', gy.permute(0, 3, 1, 2), y, my, Ci * 9, dtype)
    _within('dx', gdx.permute(0, 3, 1, 2), dx, mdx, Co * 9, dtype)
    _within('dW', gdW, dW, mdW, N * H * W, 'f32')
    P = N * H * W
    v = gy.double().reshape(P, Co)
    for row, tot, mag in ((0, v.sum(0), v.abs().sum(0)), (1, (v * v).sum(0), (v * v).sum(0))):
        assert bool(((st[row].double() - tot).abs() <= P * eb.U_ACC * mag + eb.TINY).all()), ('statistics row', row)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('N,H,W,Ci,Co,d', DILATED, ids=lambda v: str(v))
def test_dense_control_keeps_its_kernel(N, H, W, Ci, Co, d, dtype):
    """the same operands through a dense 3 x 3 (dilation 1, pad 1): correct, and served by the specialised kernels its shape
    selects (DENSE_BF16), not pushed to the general kernel by the span helper"""
    w = _randn((Co, Ci, 3, 3), 31 + d, dtype, (2.0 / (Ci * 9)) ** 0.5)
    x, dy = _randn((N, Ci, H, W), 32 + d, dtype), _randn((N, Co, H, W), 33 + d, dtype)
    (y, dx, dW), (my, mdx, mdW) = _refs(x, w, dy, 1)
    gy, st, gdx, gdW, names = _run_conv(dtype, N, H, W, Ci, Co, 1, w, x, dy)
    print('dense control %s: served by %s' % (dtype, names))
    if dtype == 'f32':
        assert names == ('kernel:fprop_general', 'kernel:fprop_general', 'kernel:wgrad_general'), names
    else:
        assert names == DENSE_BF16[(N, H, W, Ci, Co)], names
    _within('y', gy.permute(0, 3, 1, 2), y, my, Ci * 9, dtype)
    _within('dx', gdx.permute(0, 3, 1, 2), dx, mdx, Co * 9, dtype)
    _within('dW', gdW, dW, mdW, N * H * W, 'f32')


FUSED_ENTRY_POINTS = ('segnb_conv_fprop_bnreduce', 'segnb_conv_fprop_bnsums', 'segnb_conv_fprop_bnapply', 'segnb_conv_fprop_tf',
                      'segnb_conv_wgrad_tf', 'segnb_conv_wgrad_bnapply', 'segnb_conv_fprop_drop', 'segnb_conv_fprop_upcat',
                      'segnb_conv_fprop_upsum', 'segnb_conv_wgrad_upcat', 'segnb_conv_fprop_u8')


@pytest.mark.parametrize('dtype', DTYPES)
def test_dilated_conv_units_through_the_tape(dtype):
    """tests/dilated_net.py (three dilated conv_units with BatchNorm, a residual and ReLU; shapes that pass the size gates of the
    c8, rolling, resident-weight and LDS-DMA kernels and of their fused BatchNorm forms): an eval forward, then training steps in
    the same tape -- eager, recorded, replayed -- against the float64 torch function.  The census of the eager training step
    holds no fused convolution entry point and no kernel but the table walkers.
    fp32: as on the emulator (1e-4 of the logit scale, 1e-3 relative L2 per gradient).  bf16: every stored tensor is rounded to
    2^-9 relative; nine of them lie between the input and a first-layer gradient (three layers x output, normalised output,
    gradient), 9 x 2^-9 = 1.8 %, and a BatchNorm divides by a standard deviation below one -- 0.1 of the logit scale and a
    gradient cosine of 0.98 leave a factor of five."""
    import dilated_net as DN
    torch.manual_seed(2)
    m = DN.DilatedNet(num_classes=2).set_compute_dtype(dtype)
    x, G = _randn((2, 3, 32, 32), 91), _randn((2, 2, 32, 32), 92)
    ev, out, grads, bufs = DN.reference_step(m, x, G)
    m.to(DEV)
    x, G = x.to(DEV), G.to(DEV)
    ltol = 1e-4 if dtype == 'f32' else 0.1
    m.eval()
    with torch.no_grad():
        got = m(x)
    assert float((got.double().cpu() - ev).abs().max()) <= ltol * float(ev.abs().max())
    m.train()
    steps = []
    for i in range(3):
        m.zero_grad()
        if i == 0:
            with census():
                got = m(x)
                # d((logits * G).sum()) / d(logits) = G, handed to the model's backward on THIS thread: the census is per
                # thread and autograd would run the backward on its own
                m._run_backward(G.clone())
                torch.cuda.synchronize()
                seen = nv.census_read()
        else:
            got = m(x)
            (got * G).sum().backward()
            torch.cuda.synchronize()
        steps.append((got.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}))
    assert [e for e in m._tape.plans.values() if e.get('state') == 'ready'], 'the third step did not replay a recorded list'
    print('census of the eager step:', {k: v for k, v in seen.items() if k.startswith(('kernel:', 'segnb_conv'))})
    assert not [k for k in seen if k in FUSED_ENTRY_POINTS], seen
    kernels = {k for k in seen if k.startswith('kernel:')}
    assert kernels and kernels <= TABLE_WALKERS | {'kernel:wgrad_general'}, kernels
    assert seen.get('kernel:wgrad_general') == 3
    got, g1 = steps[0]
    assert float((got.double().cpu() - out).abs().max()) <= ltol * float(out.abs().max())
    if dtype == 'f32':
        for n in grads:
            rel = float((g1[n].double().cpu() - grads[n]).norm() / (grads[n].norm() + 1e-30))
            assert rel <= 1e-3, (n, rel)
        for k, b in m.named_buffers():
            if 'num_batches' in k:
                assert int(b) == 3
    else:
        a = torch.cat([g1[n].double().cpu().reshape(-1) for n in sorted(grads)])
        b = torch.cat([grads[n].reshape(-1) for n in sorted(grads)])
        cos = float((a * b).sum() / (a.norm() * b.norm()))
        print('bf16 gradient cosine %.4f' % cos)
        assert cos >= 0.98, cos
    # the recorded and the replayed step repeat the eager one (training-mode logits do not depend on the running statistics;
    # the weight gradients of the general kernel are sums of fp32 atomics: 1e-6, as in test_gcn_gpu)
    for o, g in steps[1:]:
        assert torch.equal(o, got)
        for n in g:
            assert float((g[n] - g1[n]).norm() / (g1[n].norm() + 1e-30)) <= 1e-6, n
