"""GCN34 and its decoder kernels (csrc/gcn.hip, include/segnb_gcn.h) on the MI355X:

  1. each kernel against torch autograd in float64 (F.conv2d with asymmetric padding, F.interpolate(align_corners=True)) at
     the model's shapes: C in {64, 512}, K in {1, 3, 12, 32}, 128^2 and 16^2 features, both encoder dtypes, Dropout2d
     multipliers, accumulation into existing gradients, bitwise-repeatable reductions;
  2. GCN34 fp32 against the three fixture cases (check_product_golden's tolerances);
  3. GCN34 bf16 against the fp32 restatement (gradient cosine, as check_against_oracle);
  4. two identical steps give bitwise-equal logits and decoder gradients;
  5. recorded-plan replay (step >= 3) is bitwise equal to an instance that never records;
  (4, 5: the encoder's stem and 1x1 stride-2 weight gradients run on the general weight-gradient kernel, whose fp32 atomics
  differ by ~1e-8 relative from step to step -- DESIGN.md 13.16 -- so those are held to 1e-6 instead of bitwise)
  6. two accumulating steps without zero_grad against torch accumulation;
  7. one step at K = 12 with lib.losses.JaccardLossMulti against the restatement;
  8. a 512^2 bs = 16 bf16 training run: finite, the loss goes down.
"""
import copy
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gcn_ref as R
import mc_loss_ref as MR
import model_checks as mc
import test_gcn_cpu as TC
from segnb import _native as nv

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
F64 = torch.float64


def _st():
    return torch.cuda.current_stream(DEV).cuda_stream


def _close(got, ref, rtol, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = float(ref.detach().abs().max()) + 1e-30
    err = float((got - ref).abs().max())
    assert err <= rtol * scale, '%s: max |d| %.3e of scale %.3e' % (what, err, scale)


def _randn(shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(DEV)


# ---------------------------------------------------------------------------------------------------------------- 1. kernels
GCM_SHAPES = [(64, 1, 128), (64, 3, 128), (64, 12, 128), (64, 32, 128), (512, 1, 16), (512, 3, 16), (512, 12, 16),
              (512, 32, 16)]


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('C,K,S', GCM_SHAPES, ids=lambda v: str(v))
def test_gcm_kernels_vs_autograd(C, K, S, dtype):
    N, H, W = 2, S, S
    code, tdt = (nv.F32, torch.float32) if dtype == 'f32' else (nv.BF16, torch.bfloat16)
    ld = C + 8                                               # a pixel stride wider than C, as the executor's views may have
    xbuf = _randn((N, H, W, ld), seed=1).to(tdt)
    x = xbuf[..., :C]
    drop = (torch.rand((N, C), generator=torch.Generator().manual_seed(2)) > 0.1).float().to(DEV) / 0.9
    s1, s2 = (2.0 / (C * 7)) ** 0.5, (2.0 / (K * 7)) ** 0.5
    wl1, wr1 = _randn((K, C, 7, 1), s1, 3), _randn((K, C, 1, 7), s1, 4)
    wl2, wr2 = _randn((K, K, 1, 7), s2, 5), _randn((K, K, 7, 1), s2, 6)
    bl1, br1, bl2, br2 = [_randn((K,), 0.1, 7 + i) for i in range(4)]
    yl, yr, out = [torch.empty((N, K, H, W), device=DEV) for _ in range(3)]
    P = nv.ptr
    nv.call('segnb_gcm_fwd', code, P(xbuf), ld, N, H, W, C, K, P(drop), P(wl1), P(bl1), P(wl2), P(bl2), P(wr1), P(br1), P(wr2),
            P(br2), P(yl), P(yr), P(out), _st())
    # float64 autograd on the same (dtype-rounded) feature
    leaves = [t.double().requires_grad_(True) for t in (wl1, bl1, wl2, bl2, wr1, br1, wr2, br2)]
    X = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    ro, rl, rr = R.gcm(X, drop.double(), *leaves)
    _close(yl, rl, 2e-5, 'yl')
    _close(yr, rr, 2e-5, 'yr')
    _close(out, ro, 2e-5, 'out')
    dout = _randn((N, K, H, W), seed=20)
    ro.backward(dout.double())
    dyl, dyr = torch.empty_like(yl), torch.empty_like(yr)
    dxbuf = torch.full((N, H, W, ld), 7.0, device=DEV, dtype=tdt)
    grads0 = [_randn(t.shape, 0.5, 30 + i) for i, t in enumerate((wl1, bl1, wl2, bl2, wr1, br1, wr2, br2))]
    grads = [g.clone() for g in grads0]                      # accumulated INTO (the flat.grad_of contract)

    def bwd(gs, dxb):
        nv.call('segnb_gcm_bwd', code, P(xbuf), ld, N, H, W, C, K, P(drop), P(wl1), P(wl2), P(wr1), P(wr2), P(yl), P(yr),
                P(dout), P(dyl), P(dyr), P(dxb), ld, *[P(g) for g in gs], _st())
    bwd(grads, dxbuf)
    names = ('w_l1', 'b_l1', 'w_l2', 'b_l2', 'w_r1', 'b_r1', 'w_r2', 'b_r2')
    for g, g0, leaf, n in zip(grads, grads0, leaves, names):
        _close(g - g0, leaf.grad, 5e-5, n)
    _close(dxbuf[..., :C].permute(0, 3, 1, 2), X.grad, 1e-2 if dtype == 'bf16' else 2e-5, 'dx')
    assert bool((dxbuf[..., C:] == 7.0).all()), 'dx written outside its C channels'
    # bitwise repeatable
    again = [g.clone() for g in grads0]
    dx2 = torch.full_like(dxbuf, 7.0)
    bwd(again, dx2)
    torch.cuda.synchronize()
    for a, b in zip(grads, again):
        assert torch.equal(a, b)
    assert torch.equal(dxbuf, dx2)


@pytest.mark.parametrize('K', [1, 3, 12, 32])
@pytest.mark.parametrize('S', [16, 128])
def test_brm_kernels_vs_autograd(K, S):
    N, H, W = 2, S, S
    x = _randn((N, K, H, W), seed=1)
    s = (2.0 / (K * 9)) ** 0.5
    w1, w2 = _randn((K, K, 3, 3), s, 2), _randn((K, K, 3, 3), s, 3)
    b1, b2 = _randn((K,), 0.1, 4), _randn((K,), 0.1, 5)
    r, out = torch.empty_like(x), torch.empty_like(x)
    P = nv.ptr
    nv.call('segnb_brm_fwd', N, H, W, K, P(x), P(w1), P(b1), P(w2), P(b2), P(r), P(out), _st())
    leaves = [t.double().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    ro, rr = R.brm(*leaves)
    _close(r, rr, 2e-5, 'r')
    _close(out, ro, 2e-5, 'out')
    dout = _randn((N, K, H, W), seed=6)
    ro.backward(dout.double())
    grads0 = [_randn(t.shape, 0.5, 10 + i) for i, t in enumerate((w1, b1, w2, b2))]
    grads = [g.clone() for g in grads0]
    dr, dx = torch.empty_like(x), torch.empty_like(x)
    nv.call('segnb_brm_bwd', N, H, W, K, P(x), P(w1), P(w2), P(r), P(dout), P(dr), P(dx), *[P(g) for g in grads], _st())
    _close(dx, leaves[0].grad, 2e-5, 'dx')
    for g, g0, leaf, n in zip(grads, grads0, leaves[1:], ('w1', 'b1', 'w2', 'b2')):
        _close(g - g0, leaf.grad, 5e-5, n)
    again = [g.clone() for g in grads0]
    nv.call('segnb_brm_bwd', N, H, W, K, P(x), P(w1), P(w2), P(r), P(dout), P(dr), P(dx), *[P(g) for g in again], _st())
    torch.cuda.synchronize()
    for a, b in zip(grads, again):
        assert torch.equal(a, b)


@pytest.mark.parametrize('N,K,h,w,H,W,skip', [(2, 1, 256, 256, 512, 512, False), (2, 3, 32, 32, 80, 80, True),
                                              (16, 1, 16, 16, 32, 32, True), (2, 12, 128, 128, 256, 256, False),
                                              (1, 32, 32, 48, 80, 72, True), (1, 2, 40, 40, 24, 24, False)])
def test_resize_kernels_vs_autograd(N, K, h, w, H, W, skip):
    a = _randn((N, K, h, w), seed=1)
    sk = _randn((N, K, H, W), seed=2) if skip else None
    out = torch.empty((N, K, H, W), device=DEV)
    P = nv.ptr
    nv.call('segnb_resize_bilinear_ac_fwd', N, K, h, w, P(a), H, W, P(sk), P(out), _st())
    A = a.double().requires_grad_(True)
    ref = R.resize(A, (H, W), sk.double() if skip else None)
    _close(out, ref, 1e-5, 'resize')
    g = _randn((N, K, H, W), seed=3)
    ref.backward(g.double())
    din = torch.empty_like(a)
    nv.call('segnb_resize_bilinear_ac_bwd', N, K, h, w, H, W, P(g), P(din), _st())
    _close(din, A.grad, 1e-5, 'resize backward')


def test_out_of_range_is_refused():
    assert nv.query('segnb_gcn_ok', 64, 33, 1, 8, 8) == 0 and nv.query('segnb_gcn_ok', 60, 1, 1, 8, 8) == 0
    a = torch.zeros((1, 33, 8, 8), device=DEV)
    with pytest.raises(RuntimeError):
        nv.call('segnb_resize_bilinear_ac_fwd', 1, 33, 8, 8, nv.ptr(a), 8, 8, None, nv.ptr(torch.empty_like(a)), _st())


# ---------------------------------------------------------------------------------------------------------------- 2.-8. model
@pytest.mark.parametrize('prefix', sorted(TC.CASES))
def test_gcn34_fp32_vs_reference_fixture(prefix):
    g = TC.load_case(prefix)
    m = TC.make_gcn(prefix, g)
    if prefix == 'k3':
        TC.check_dot_case(m, g, DEV)
    else:
        mc.check_product_golden(m, g, DEV)


def _seeded(K=1, size=64, seed=5):
    g = {'seed': np.asarray(seed)}
    from lib.models.gcn import GCN34
    from oracle import fill
    m = GCN34(num_classes=K, input_size=size, pretrained=False)
    for gm in (m.gcm1, m.gcm2, m.gcm3, m.gcm4):
        gm.pre_drop.p = 0.0
    m.load_state_dict(fill.seeded_state(m.state_dict(), int(g['seed'])))
    return m


def test_gcn34_bf16_vs_restatement():
    m = _seeded()
    x, y = mc.blob_batch(2, 64, 7)
    cos = mc.check_against_oracle(m, lambda sd, xx: R.forward(sd, xx, 64), x, y, DEV, dtype='bf16')
    # (check_against_oracle's own bf16 bound is 0.5; measured 0.89 here: the bf16 encoder's BatchNorm layers re-normalise
    # bf16-rounded tensors at random init, the fp32 decoder adds no rounding of its own -- its kernels are checked in fp32 above)
    assert cos > 0.8, cos


def _same_grads(g1, g2):
    for n in g1:
        if n.startswith(('gcm', 'brm')):
            assert torch.equal(g1[n], g2[n]), n
        else:
            err = float((g1[n] - g2[n]).norm() / (g1[n].norm() + 1e-30))
            assert err <= 1e-6, (n, err)


def _step(m, x, y, zero=True):
    from lib.losses import BCEWithLogitsLossAndSmoothJaccard
    if zero:
        m.zero_grad()
    out = m(x)
    loss = BCEWithLogitsLossAndSmoothJaccard()(out, y)
    (x.shape[0] * loss).backward()
    torch.cuda.synchronize()
    return out.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_two_identical_steps_are_bitwise_equal(dtype):
    m = _seeded().set_compute_dtype(dtype).to(DEV).train()
    x, y = mc.blob_batch(2, 64, 8)
    x, y = x.to(DEV), y.to(DEV)
    o1, g1 = _step(m, x, y)
    o2, g2 = _step(m, x, y)
    assert torch.equal(o1, o2)
    _same_grads(g1, g2)


def test_replayed_steps_equal_an_instance_that_never_records():
    a = _seeded(K=3, size=(64, 96)).set_compute_dtype('bf16').to(DEV).train()
    b = copy.deepcopy(a)
    b.use_cplan = False
    x, _ = mc.blob_batch(2, 64, 9)
    x = x.to(DEV)
    G = _randn((2, 3, 64, 96), seed=11)

    def step(m):
        m.zero_grad()
        out = m(x)
        (out * G).sum().backward()
        torch.cuda.synchronize()
        return out.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    for _ in range(3):
        oa, ga = step(a)
    ent = [e for e in a._tape.plans.values() if e.get('state') == 'ready']
    assert ent, 'the third step did not replay a recorded list'
    ob, gb = step(b)
    assert torch.equal(oa, ob)
    _same_grads(ga, gb)


def _restated_grads(m, xs, ys, K, size):
    from oracle import losses_ref
    sd = {k: v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone() for k, v in m.state_dict().items()}
    pn = [n for n, _ in m.named_parameters()]
    leaves = {k: (v.clone().requires_grad_(True) if k in pn else v.clone()) for k, v in sd.items()}
    for x, y in zip(xs, ys):
        lo = R.forward(leaves, x.double(), size)
        (x.shape[0] * losses_ref.bce_jaccard(lo, y)).backward()
    return {n: leaves[n].grad for n in pn}


def _grad_agreement(got, ref, min_cos):
    names = sorted(ref)
    ga = torch.cat([got[n].double().cpu().reshape(-1) for n in names])
    gr = torch.cat([ref[n].reshape(-1) for n in names])
    cos = float((ga * gr).sum() / (ga.norm() * gr.norm()))
    assert cos > min_cos, cos
    for n in names:
        if float(ref[n].abs().max()) > 1e-7 * float(gr.abs().max()):
            rel = float((got[n].double().cpu() - ref[n]).norm() / (ref[n].norm() + 1e-30))
            assert rel <= 0.1, (n, rel)


def test_two_accumulating_steps_without_zero_grad():
    m = _seeded().set_compute_dtype('f32').to(DEV).train()
    (x1, y1), (x2, y2) = mc.blob_batch(2, 64, 12), mc.blob_batch(2, 64, 13)
    ref = _restated_grads(m, [x1, x2], [y1, y2], 1, 64)
    m.zero_grad()
    _step(m, x1.to(DEV), y1.to(DEV), zero=False)
    _, got = _step(m, x2.to(DEV), y2.to(DEV), zero=False)
    _grad_agreement(got, ref, 0.9999)


def test_k12_step_with_jaccard_loss_multi():
    from lib.losses import JaccardLossMulti
    m = _seeded(K=12).set_compute_dtype('f32').to(DEV).train()
    x, _ = mc.blob_batch(2, 64, 14)
    t = torch.randint(0, 12, (2, 64, 64), generator=torch.Generator().manual_seed(15))
    crit = JaccardLossMulti()
    sd = {k: v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone() for k, v in m.state_dict().items()}
    pn = [n for n, _ in m.named_parameters()]
    leaves = {k: (v.clone().requires_grad_(True) if k in pn else v.clone()) for k, v in sd.items()}
    lo = R.forward(leaves, x.double(), 64)
    cfg, nw, jw = MR.cfg_of(crit)
    rloss, _, dlog = MR.loss_and_grad(lo.detach(), t, cfg, nw, jw)
    lo.backward(dlog)
    m.zero_grad()
    out = m(x.to(DEV))
    loss = crit(out, t.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - float(rloss)) < 1e-4, (loss.item(), float(rloss))
    _grad_agreement({n: p.grad for n, p in m.named_parameters()}, {n: leaves[n].grad for n in pn}, 0.9999)


def test_512_bs16_bf16_training_loss_goes_down():
    from lib.losses import BCEWithLogitsLossAndSmoothJaccard
    from lib.models.gcn import GCN34
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = GCN34(num_classes=1, input_size=512).to(DEV).train()
    x, y = mc.blob_batch(16, 512, 16)
    x, y = x.to(DEV), y.to(DEV)
    opt = torch.optim.SGD(m.parameters(), lr=1e-2, momentum=0.9)
    crit = BCEWithLogitsLossAndSmoothJaccard()
    losses = []
    for _ in range(6):
        opt.zero_grad()
        out = m(x)
        loss = crit(out, y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(np.isfinite(losses)), losses
    assert all(torch.isfinite(p).all() for p in m.parameters())
    assert losses[-1] < losses[0], losses
