"""The multi-class losses and the 9-32 class heads on the MI355X (csrc/mc_loss.hip, csrc/head_loss.hip):
fixture cases of the reference through lib.losses, large batches against the float64 restatement (tests/mc_loss_ref.py),
bitwise reproducibility, the one- vs two-launch forms, heads with K = 9 .. 32 against torch, and one-step model gradients
at K > 1 against the oracle forwards."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mc_loss_ref as R
from test_mc_loss_cpu import CASES, check_case, make_module

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%d-%s-C%d' % (c[0], c[1]['cls'], c[2].shape[1]))
def test_fixture_case_on_hip(case):
    i, cfg, x, t, up, ref_loss, ref_grad = case
    xr = x.to(DEV).requires_grad_(True)
    loss = make_module(cfg)(xr, t.to(DEV))
    (loss * up.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    check_case(loss.detach(), xr.grad, ref_loss, ref_grad)


def _batch(N, C, H, W, seed, bad=False, offset=0):
    g = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(N * C * H * W + offset, generator=g)
    t = torch.randint(0, C, (N, H, W), generator=g)
    if C > 3:
        t[t == 2] = 0                                   # a class absent from the targets
    t[torch.rand(N, H, W, generator=g) < 0.1] = -1
    if bad:
        t[0, 0, :5] = C + 3
        t[-1, -1, -3:] = -7
    xd = x.to(DEV)[offset:].view(N, C, H, W)          # offset 1: a logits pointer that is not 16-byte aligned
    return xd, t.to(DEV)


def _run(mod, x, t, up=None):
    from segnb.mcloss import mc_loss
    xr = x.detach().clone() if x.data_ptr() % 16 == 0 else x.detach()
    xr.requires_grad_(True)
    loss = mod(xr, t)
    fin = mc_loss.last_fin.clone()
    (loss if up is None else (loss * up).sum()).backward()
    torch.cuda.synchronize()
    return loss.detach(), xr.grad.detach(), fin


@pytest.mark.parametrize('C', [2, 4, 12, 21, 150])
def test_large_batch_against_the_restatement(C):
    from lib.losses import FocalAndJaccardLossMulti, NLLLAndJaccardLossMulti, JaccardLossMulti
    N = 32 if C <= 21 else 8
    x, t = _batch(N, C, 224, 224, seed=C, bad=True)
    wts = np.linspace(0.5, 2.0, C)
    for mod in (FocalAndJaccardLossMulti(jaccard_weight=0.5, class_weights=wts), NLLLAndJaccardLossMulti(class_weights=wts),
                JaccardLossMulti(ignore_index=-1, weight=torch.tensor(wts, dtype=torch.float32), reduce=False)):
        up = None if mod.__class__.__name__ != 'JaccardLossMulti' else torch.rand(C, device=DEV) + 0.5
        loss, dx, fin = _run(mod, x, t, up)
        c, nw, jw = R.cfg_of(mod)
        rl, rfin, rdx = R.loss_and_grad(x, t, c, nw, jw, gout=up)
        assert torch.allclose(loss.double(), rl, rtol=1e-5, atol=1e-7), (mod, loss, rl)
        # (logits of magnitude ~10: the fp32 log-sum-exp alone puts ~1e-6 absolute error on logp, i.e. ~2e-6 of the largest
        # gradient entry -- the fixture cases hold the binary family's 2e-6 bound, these fp32-vs-fp64 ones 1e-5)
        assert torch.allclose(dx.double(), rdx, rtol=1e-4, atol=1e-5 * float(rdx.abs().max())), float((dx.double() - rdx).abs().max())
        assert float(fin[5]) == 8.0 and float(fin[4]) == N * 224 * 224 and float(fin[3]) == float(rfin[3])
        del dx, rdx


@pytest.mark.parametrize('C,H,W,offset', [(5, 37, 41, 0), (12, 30, 30, 1), (40, 17, 19, 1), (3, 224, 224, 1)])
def test_scalar_tails_and_unaligned_pointers(C, H, W, offset):
    from lib.losses import FocalAndJaccardLossMulti
    x, t = _batch(3, C, H, W, seed=7 + C, bad=True, offset=offset)
    mod = FocalAndJaccardLossMulti(jaccard_weight=2)
    loss, dx, fin = _run(mod, x, t)
    c, nw, jw = R.cfg_of(mod)
    rl, rfin, rdx = R.loss_and_grad(x, t, c, nw, jw)
    assert torch.allclose(loss.double(), rl, rtol=1e-5)
    assert torch.allclose(dx.double(), rdx, rtol=1e-4, atol=1e-5 * float(rdx.abs().max()))
    assert float(fin[5]) == 8.0


@pytest.mark.parametrize('C', [4, 21, 150])
def test_reproducible_and_one_launch_equals_two(C, monkeypatch):
    from lib.losses import FocalAndJaccardLossMulti
    from segnb import mcloss
    x, t = _batch(32 if C < 150 else 8, C, 224, 224, seed=3 * C)
    mod = FocalAndJaccardLossMulti(jaccard_weight=0.5)
    a = _run(mod, x, t)
    b = _run(mod, x, t)
    monkeypatch.setattr(mcloss, '_ONE_LAUNCH', False)
    c = _run(mod, x, t)
    for u, v in ((a, b), (a, c)):
        assert torch.equal(u[0], v[0]) and torch.equal(u[2], v[2]) and torch.equal(u[1], v[1])


# ------------------------------------------------------------------------------------------------------------------ heads
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('shape', [(2, 9, 13, 20, 9), (2, 16, 16, 32, 12), (1, 7, 9, 64, 32), (2, 6, 10, 256, 12),
                                   (1, 5, 7, 272, 32)])
def test_head_many_classes(shape, dtype):
    from segnb import convplan as cp
    from test_hip_ops import Runtime, View, check
    from segnb import _native as nv
    N, H, W, C, K = shape
    Cp = cp.pad8(C)
    gen = torch.Generator().manual_seed(C + K)
    a = torch.randn(N, H, W, C, generator=gen)
    w = torch.randn(K, C, 1, 1, generator=gen) * 0.2
    b = torch.randn(K, generator=gen)
    dl = torch.randn(N, K, H, W, generator=gen)
    if dtype == 'bf16':
        a = a.bfloat16().float()
    rt = Runtime('cuda', dtype)
    av = View.alloc(rt, N, H, W, Cp)
    av.dense()[..., :C] = a.to(rt.device, rt.tdtype)
    wd, bd, dld = w.to(rt.device), b.to(rt.device), dl.to(rt.device)
    logits = torch.zeros(N, K, H, W, device=rt.device)
    nv.call('segnb_head_fwd', rt.code, av.ptr, av.ld, N, H, W, C, nv.ptr(wd), nv.ptr(bd), K, nv.ptr(logits), rt.stream)
    da = View.alloc(rt, N, H, W, Cp)
    dw, db = torch.zeros_like(wd), torch.zeros_like(bd)
    nv.call('segnb_head_bwd', rt.code, av.ptr, av.ld, N, H, W, C, Cp, nv.ptr(wd), K, nv.ptr(dld), da.ptr, da.ld, nv.ptr(dw),
            nv.ptr(db), rt.stream)
    torch.cuda.synchronize()
    ar = a.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    out = F.conv2d(ar, wr, br)
    out.backward(dl)
    check('logits vs torch', logits.cpu(), out, 'f32')
    check('da vs torch', da.dense().float().cpu()[..., :C].permute(0, 3, 1, 2), ar.grad, dtype)
    check('dw vs torch', dw.cpu(), wr.grad, 'f32')
    check('db vs torch', db.cpu(), br.grad, 'f32')


# ------------------------------------------------------------------------------------------------------------ model level
def _oracle_step(forward, sd, pnames, x, t, mod, dtype):
    c, nw, jw = R.cfg_of(mod)
    leaves = {k: (v.clone().to(dtype).requires_grad_(True) if k in pnames else
                  (v.clone().to(dtype) if v.is_floating_point() else v.clone())) for k, v in sd.items()}
    logits = forward(leaves, x.to(dtype))
    loss = R.finalize(R.sums(logits, t, c, nw), logits.shape[1], c, jw)[0]
    (x.shape[0] * loss).backward()
    return logits.detach(), loss.item(), {k: leaves[k].grad.double() for k in pnames}


def check_mc_against_oracle(model, forward, x, t, mod, min_cos=0.9999):
    B = x.shape[0]
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    pnames = set(n for n, _ in model.named_parameters())
    lo64, loss64, g64 = _oracle_step(forward, sd, pnames, x, t, mod, torch.float64)
    _, _, g32 = _oracle_step(forward, sd, pnames, x, t, mod, torch.float32)
    model.set_compute_dtype('f32')
    model.to(DEV).train()
    out = model(x.to(DEV))
    loss = mod(out, t.to(DEV))
    (B * loss).backward()
    torch.cuda.synchronize()
    scale = float(lo64.abs().max())
    assert float((out.detach().cpu().double() - lo64).abs().max()) <= 1e-3 * scale
    assert abs(loss.item() - loss64) <= 1e-4 * abs(loss64), (loss.item(), loss64)
    got = {n: p.grad.detach().cpu().double() for n, p in model.named_parameters()}
    ga = torch.cat([got[n].reshape(-1) for n in sorted(pnames)])
    gr = torch.cat([g64[n].reshape(-1) for n in sorted(pnames)])
    cos = float((ga * gr).sum() / (ga.norm() * gr.norm()))
    # noise-aware, as check_against_oracle: random-init BatchNorm nets amplify fp32 summation noise on the way back, so the
    # bound is the larger of 1 - min_cos and a few times the fp32 oracle's own distance from fp64
    g3 = torch.cat([g32[n].reshape(-1) for n in sorted(pnames)])
    cos32 = float((g3 * gr).sum() / (g3.norm() * gr.norm()))
    assert 1 - cos <= max(1 - min_cos, 10 * (1 - cos32)), (cos, cos32)
    print('gradient cosine vs fp64 oracle: product %.7f, fp32 oracle %.7f' % (cos, cos32))
    return cos


def _targets(B, K, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, K, (B, H, W), generator=g)
    t[torch.rand(B, H, W, generator=g) < 0.1] = -1
    return t


@pytest.mark.parametrize('K', [4, 6, 12])
def test_zf_unet_multiclass_step_vs_oracle(K):
    from lib.models.zf_unet import ZF_UNET
    from lib.losses import FocalAndJaccardLossMulti
    from oracle import zf_unet_ref
    torch.manual_seed(K)
    m = ZF_UNET(dropout_val=0.0, filters=8, num_classes=K)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, 64, 64, generator=g)
    check_mc_against_oracle(m, lambda sd, xx: zf_unet_ref.forward(sd, xx, True), x, _targets(2, K, 64, 64, K),
                            FocalAndJaccardLossMulti(jaccard_weight=0.5))


def test_fcdensenet57_twelve_classes_step_vs_oracle():
    from lib.models.tiramisu import FCDenseNet57
    from lib.losses import NLLLAndJaccardLossMulti
    from oracle import tiramisu_ref
    torch.manual_seed(3)
    m = FCDenseNet57(n_classes=12)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout2d):
            mod.p = 0.0
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(4))
    fwd = lambda sd, xx: tiramisu_ref.forward(sd, xx, (4, 4, 4, 4, 4), (4, 4, 4, 4, 4), 4, True)
    check_mc_against_oracle(m, fwd, x, _targets(2, 12, 32, 32, 5), NLLLAndJaccardLossMulti(jaccard_weight=0.5), min_cos=0.999)


def test_unet16_twelve_classes_step_vs_oracle():
    from lib.models.unet16 import UNet16
    from lib.losses import FocalAndJaccardLossMulti
    from oracle import unet16_ref
    torch.manual_seed(0)
    m = UNet16(num_filters=8, num_classes=12)
    x = torch.randn(2, 3, 32, 64, generator=torch.Generator().manual_seed(1))
    check_mc_against_oracle(m, unet16_ref.forward, x, _targets(2, 12, 32, 64, 2), FocalAndJaccardLossMulti(), min_cos=0.999)


def test_fcdensenet67_twelve_classes_trains_a_step():
    from lib.models.tiramisu import FCDenseNet67
    from lib.losses import FocalAndJaccardLossMulti
    torch.manual_seed(0)
    m = FCDenseNet67(n_classes=12).to(DEV).train()
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    x = torch.randn(2, 3, 64, 64, device=DEV)
    t = _targets(2, 12, 64, 64, 9).to(DEV)
    out = m(x)
    assert out.shape == (2, 12, 64, 64)
    loss = FocalAndJaccardLossMulti()(out, t)
    (2 * loss).backward()
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()
    assert all(torch.isfinite(p.grad).all().item() for p in m.parameters() if p.grad is not None)


def test_train_epoch_with_multiclass_loss():
    import torch_train
    from lib.models.zf_unet import ZF_UNET
    from lib.losses import FocalAndJaccardLossMulti
    torch.manual_seed(1)
    m = ZF_UNET(dropout_val=0.0, filters=8, num_classes=12).to(DEV).train()
    g = torch.Generator().manual_seed(2)
    data = [(torch.randn(2, 3, 64, 64, generator=g), _targets(2, 12, 64, 64, s)) for s in range(3)]
    opt = torch.optim.SGD(m.parameters(), lr=1e-2)
    losses, _ = torch_train.train(m, FocalAndJaccardLossMulti(), opt, data)
    assert losses.count == 3 * 2 or losses.count == 3
    assert np.isfinite(losses.avg)
