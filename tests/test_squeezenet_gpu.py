"""SqueezeNet and the ELU passes (csrc/elu.hip, include/segnb_elu.h) on the MI355X:

  1. the kernels against float64 torch on the same storage-rounded inputs: both dtypes, in place and out of place, with and
     without the upsample-add, one / two / three gradient sources, one and two sums tables, pixel strides wider than the
     channels (sentinels), bit-equal repeats;
  2. the fused upsample-add launch is bit-equal to the ELU pass + a nearest copy + segnb_add, at the operator level;
  3. SqueezeNet fp32 against the two fixture cases (check_product_golden's tolerances);
  4. SqueezeNet bf16 against the restatement (gradient cosine), held to torch's own bf16 autocast of the restatement;
  5. two identical steps, recorded-plan replay against an instance that never records, two accumulating steps;
  6. the producer protocol on a two-layer net, and its fallback;
  7. a 64^2 bs = 8 bf16 SGD run: finite, the loss goes down.
"""
import copy

import numpy as np
import pytest
import torch

import model_checks as mc
import squeezenet_ref as R
import test_squeezenet_cpu as TC
from segnb import _native as nv

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
F64 = torch.float64
REPL = 16                                   # SEGNB_STAT_REPLICAS
SENTINEL = 7.0


def _st():
    return torch.cuda.current_stream(DEV).cuda_stream


def _dt(dtype):
    return (nv.F32, torch.float32) if dtype == 'f32' else (nv.BF16, torch.bfloat16)


def _buf(N, H, W, Cp, ld, tdt, seed, scale):
    """[N, H, W, ld] buffer: N(0, scale^2) in channels [0, Cp), SENTINEL in [Cp, ld)"""
    g = torch.Generator().manual_seed(seed)
    t = torch.full((N, H, W, ld), SENTINEL, dtype=torch.float32)
    t[..., :Cp] = torch.randn((N, H, W, Cp), generator=g) * scale
    return t.to(tdt).to(DEV)


def _plant(z, Cp):
    """exact 0, +-1e-4, -100, +100 in every channel (cyclically over the first pixels and the channels)"""
    vals = torch.tensor([0.0, 1e-4, -1e-4, -100.0, 100.0])
    flat = z.view(-1, z.shape[-1])
    npl = min(5, flat.shape[0])
    c = torch.arange(Cp)
    for p in range(npl):
        flat[p, :Cp] = vals[(p + c) % 5].to(z.dtype).to(z.device)
    if flat.shape[0] < 5:                   # a single pixel: the five values across its channels
        flat[0, :Cp] = vals[c % 5].to(z.dtype).to(z.device)


def _assert_bound(got, ref, dtype, what):
    """f32: 3 ulp of expm1f / two fp32 roundings; bf16: one rounding to bf16 on top (half an ulp is 2^-9)"""
    got, ref = got.double().cpu(), ref.double().cpu()
    rel, floor = (4e-7, 1e-7) if dtype == 'f32' else (2.0 ** -8, 2.0 ** -133)
    over = (got - ref).abs() - (rel * ref.abs() + floor)
    assert float(over.max()) <= 0.0, '%s: |d| exceeds the bound by %.3e (at ref %.6e)' % (what, float(over.max()),
                                                                                          float(ref.reshape(-1)[over.argmax()]))


def _sentinel_kept(t, Cp, what):
    if t.shape[-1] > Cp:
        assert bool((t[..., Cp:].float() == SENTINEL).all()), what + ': channels [Cp, ld) were written'


# ---------------------------------------------------------------------------------------------------------------- 1. kernels
# (the last one: 262 144 pixels of 8 chunk columns -- 8192+ trips against a grid capped at 8 blocks per CU, so every block
# walks its grid-stride loop several times and many blocks add into each sums replica)
SHAPES = [(1, 1, 1, 8, 8), (2, 5, 7, 16, 24), (2, 12, 20, 48, 176), (1, 3, 5, 1024, 1024), (3, 9, 9, 128, 128),
          (16, 128, 128, 64, 64)]


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('N,H,W,Cp,ld', SHAPES, ids=lambda v: str(v))
def test_elu_forward_vs_float64(N, H, W, Cp, ld, dtype):
    code, tdt = _dt(dtype)
    assert nv.query('segnb_elu_ok', code, N, H, W, Cp) == 1
    z = _buf(N, H, W, Cp, ld, tdt, 1, 2.0)
    _plant(z, Cp)
    zf = z[..., :Cp].double()
    ref = torch.where(zf > 0, zf, torch.expm1(zf))
    skip = _buf(N, 2 * H, 2 * W, Cp, ld, tdt, 2, 1.0)
    P = nv.ptr
    for inplace in (False, True):
        for with_up in (False, True):
            src = z.clone()
            a = src if inplace else torch.full_like(z, SENTINEL)
            up = torch.full_like(skip, SENTINEL) if with_up else None
            nv.call('segnb_elu_fwd', code, P(src), ld, N, H, W, Cp, P(a), ld, P(skip) if with_up else None, ld, P(up), ld, _st())
            torch.cuda.synchronize()
            what = 'a (in place %s, up %s)' % (inplace, with_up)
            _assert_bound(a[..., :Cp], ref, dtype, what)
            _sentinel_kept(a, Cp, what)
            if not inplace:
                assert torch.equal(src, z), 'the source of an out-of-place pass was written'
            if with_up:
                rep = a[..., :Cp].float().repeat_interleave(2, 1).repeat_interleave(2, 2)
                want = (rep + skip[..., :Cp].float()).to(tdt)
                assert torch.equal(up[..., :Cp], want), 'up_out is not rnd(float(a) + float(skip)) bit for bit'
                _sentinel_kept(up, Cp, 'up_out')
    # up_out aliasing up_skip
    acc = skip.clone()
    a = torch.full_like(z, SENTINEL)
    nv.call('segnb_elu_fwd', code, P(z), ld, N, H, W, Cp, P(a), ld, P(acc), ld, P(acc), ld, _st())
    torch.cuda.synchronize()
    rep = a[..., :Cp].float().repeat_interleave(2, 1).repeat_interleave(2, 2)
    assert torch.equal(acc[..., :Cp], (rep + skip[..., :Cp].float()).to(tdt))


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('N,H,W,Cp,ld', SHAPES, ids=lambda v: str(v))
def test_elu_backward_vs_float64(N, H, W, Cp, ld, dtype):
    code, tdt = _dt(dtype)
    z = _buf(N, H, W, Cp, ld, tdt, 3, 2.0)
    _plant(z, Cp)
    a = z.clone()
    P = nv.ptr
    nv.call('segnb_elu_fwd', code, P(a), ld, N, H, W, Cp, P(a), ld, None, 0, None, 0, _st())
    gd, ga = _buf(N, H, W, Cp, ld, tdt, 4, 1.0), _buf(N, H, W, Cp, ld, tdt, 5, 1.0)
    gu = _buf(N, 2 * H, 2 * W, Cp, ld, tdt, 6, 1.0)
    C0p = 64 if Cp == 128 else Cp                                   # (3, 9, 9, 128): the sums split over two tables
    af = a[..., :Cp].double()
    dact = torch.where(af > 0, torch.ones_like(af), af + 1.0)
    for nsrc in (1, 2, 3):
        srcs = [gd, ga if nsrc >= 2 else None, gu if nsrc == 3 else None]
        # g: the fp32 sum in the header's order; the reference takes it to float64 and applies the derivative there
        g = gd[..., :Cp].float()
        if nsrc >= 2:
            g = g + ga[..., :Cp].float()
        if nsrc == 3:
            g = g + R.gather_up(gu[..., :Cp])
        ref = g.double() * dact
        s0 = torch.zeros((REPL, 2, C0p), dtype=F64, device=DEV)
        s1 = torch.zeros((REPL, 2, Cp - C0p), dtype=F64, device=DEV) if C0p < Cp else None
        for t in (s0, s1):
            if t is not None:
                t[:, 1] = 3.0
        # one source: dz aliases g_direct (a copy of it)
        dz = gd.clone() if nsrc == 1 else torch.full_like(z, SENTINEL)
        first = dz if nsrc == 1 else gd
        nv.call('segnb_elu_bwd', code, P(a), ld, N, H, W, Cp, P(first), ld, P(srcs[1]), ld, P(srcs[2]), ld, P(dz), ld, P(s0), C0p,
                P(s1), _st())
        torch.cuda.synchronize()
        what = 'dz (%d sources)' % nsrc
        _assert_bound(dz[..., :Cp], ref, dtype, what)
        _sentinel_kept(dz, Cp, what)
        stored = dz[..., :Cp].double().reshape(-1, Cp)
        tol = 1e-12 * float(stored.abs().sum())
        want = stored.sum(0)
        got = s0[:, 0].sum(0) if s1 is None else torch.cat([s0[:, 0].sum(0), s1[:, 0].sum(0)])
        assert float((got - want).abs().max()) <= tol, (what, float((got - want).abs().max()), tol)
        for t in (s0, s1):
            if t is not None:
                assert bool((t[:, 1] == 3.0).all()), 'row 1 of the sums table was written'
        # the same launch again, without sums: bit-equal dz
        dz2 = torch.full_like(z, SENTINEL)
        nv.call('segnb_elu_bwd', code, P(a), ld, N, H, W, Cp, P(gd), ld, P(srcs[1]), ld, P(srcs[2]), ld, P(dz2), ld, None, 0, None,
                _st())
        torch.cuda.synchronize()
        assert torch.equal(dz2[..., :Cp], dz[..., :Cp]), what + ': a second launch differs'
    # a source other than g_direct alone
    dz = torch.full_like(z, SENTINEL)
    nv.call('segnb_elu_bwd', code, P(a), ld, N, H, W, Cp, None, 0, None, 0, P(gu), ld, P(dz), ld, None, 0, None, _st())
    torch.cuda.synchronize()
    _assert_bound(dz[..., :Cp], R.gather_up(gu[..., :Cp]).double() * dact, dtype, 'dz (g_up alone)')


def test_out_of_range_is_refused():
    assert nv.query('segnb_elu_ok', nv.BF16, 1, 4, 4, 1032) == 0 and nv.query('segnb_elu_ok', nv.BF16, 1, 4, 4, 12) == 0
    t = torch.zeros((1, 4, 4, 16), device=DEV)
    with pytest.raises(RuntimeError):
        nv.call('segnb_elu_fwd', nv.F32, nv.ptr(t), 16, 1, 4, 4, 12, nv.ptr(t), 16, None, 0, None, 0, _st())
    with pytest.raises(RuntimeError):             # no gradient source
        nv.call('segnb_elu_bwd', nv.F32, nv.ptr(t), 16, 1, 4, 4, 16, None, 0, None, 0, None, 0, nv.ptr(torch.empty_like(t)), 16,
                None, 0, None, _st())


# ---------------------------------------------------------------------------------------------------------------- 2. fused = unfused
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_fused_upsample_add_equals_the_unfused_composition(dtype, monkeypatch):
    """elu(up_skip=...) at (2, 6, 10, 96) in the probe net (tests/test_squeezenet_cpu.py) against segnb_elu_fwd alone, a torch
    nearest copy and segnb_add on the same tensors; in fp32 the step's gradients against float64 as well (bf16: the pooling in
    front of the ELU routes by bf16 ties, check_probe_net)."""
    code, tdt = _dt(dtype)
    m, _ = TC.check_probe_net('upskip', DEV, monkeypatch, dtype=dtype, rtol=1e-4 if dtype == 'f32' else 3e-2,
                              check_grads=dtype == 'f32')
    torch.cuda.synchronize()
    pv = m.probe
    z, a, up, skip = (pv[k].dense() for k in ('z', 'a', 'up', 'skip'))
    assert tuple(a.shape) == (2, 6, 10, 96) and tuple(up.shape) == (2, 12, 20, 96)
    a2 = torch.empty((2, 6, 10, 96), dtype=tdt, device=DEV)
    P = nv.ptr
    nv.call('segnb_elu_fwd', code, pv['z'].ptr, pv['z'].ld, 2, 6, 10, 96, P(a2), 96, None, 0, None, 0, _st())
    rep = a2.repeat_interleave(2, 1).repeat_interleave(2, 2).contiguous()
    up2 = torch.empty_like(rep)
    nv.call('segnb_add', code, P(rep), 96, pv['skip'].ptr, pv['skip'].ld, P(up2), 96, 2, 12, 20, 96, _st())
    torch.cuda.synchronize()
    assert torch.equal(a2, a) and torch.equal(up2, up)


# ---------------------------------------------------------------------------------------------------------------- 3. fp32 model
@pytest.mark.parametrize('prefix', TC.CASES)
def test_squeezenet_fp32_vs_reference_fixture(prefix):
    g = TC.load_case(prefix)
    m = TC.make_squeezenet(g)
    if prefix == 'ns':
        TC.check_dot_case(m, g, DEV)
    else:
        mc.check_product_golden(m, g, DEV)


# ---------------------------------------------------------------------------------------------------------------- 4. bf16 model
def _seeded(seed=5):
    from lib.models.squeezenet import SqueezeNet
    from oracle import fill
    m = SqueezeNet()
    m.load_state_dict(fill.seeded_state(m.state_dict(), seed))
    return m


def _restated_grads(m, xs, ys, dtype=F64, autocast=False):
    from oracle import losses_ref
    sd = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in m.state_dict().items()}
    for x, y in zip(xs, ys):
        with torch.autocast('cpu', dtype=torch.bfloat16, enabled=autocast):
            lo = R.forward(sd, x.to(dtype))
        (x.shape[0] * losses_ref.bce_jaccard(lo.to(dtype), y)).backward()
    return {n: sd[n].grad.double() for n in sd}


def _cos(ga, gb):
    names = sorted(gb)
    a = torch.cat([ga[n].double().cpu().reshape(-1) for n in names])
    b = torch.cat([gb[n].double().cpu().reshape(-1) for n in names])
    return float((a * b).sum() / (a.norm() * b.norm()))


def test_squeezenet_bf16_vs_restatement():
    """Gradient cosine against the float64 restatement, as check_against_oracle (its own bf16 bound: 0.5).  That bound was set
    for BatchNorm networks; SqueezeNet has 26 consecutive activations and no normalisation, so the product is also held to a
    yardstick measured in the test: torch's bf16 autocast of the restatement on the same weights and batch must be no closer to
    float64 than the product is.  Measured on MI355X (profiles/squeezenet_ab.txt): product 0.999685, yardstick 0.999684."""
    m = _seeded()
    x, y = mc.blob_batch(2, 64, 7)
    cos = mc.check_against_oracle(m, R.forward, x, y, DEV, dtype='bf16')
    got = {n: p.grad.detach().cpu().double() for n, p in m.named_parameters()}
    g64 = _restated_grads(m, [x], [y])
    yard = _cos(_restated_grads(m, [x], [y], torch.float32, autocast=True), g64)
    prod = _cos(got, g64)
    print('bf16 gradient cosine against float64: product %.6f (check_against_oracle %.6f), autocast yardstick %.6f' % (prod, cos, yard))
    assert 1.0 - prod <= 1.0 - yard, (prod, yard)


# ---------------------------------------------------------------------------------------------------------------- 5. determinism, replay
def _step(m, x, y, zero=True):
    from lib.losses import BCEWithLogitsLossAndSmoothJaccard
    if zero:
        m.zero_grad()
    out = m(x)
    loss = BCEWithLogitsLossAndSmoothJaccard()(out, y)
    (x.shape[0] * loss).backward()
    torch.cuda.synchronize()
    return out.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def _same_grads(g1, g2):
    """bit-equal, except where the general weight-gradient kernel sums with fp32 atomics: 1e-6 relative"""
    for n in g1:
        if not torch.equal(g1[n], g2[n]):
            err = float((g1[n] - g2[n]).norm() / (g1[n].norm() + 1e-30))
            assert n.endswith('.weight') and err <= 1e-6, (n, err)


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
    a = _seeded().set_compute_dtype('bf16').to(DEV).train()
    b = copy.deepcopy(a)
    b.use_cplan = False
    x, y = mc.blob_batch(2, 64, 9)
    x, y = x.to(DEV), y.to(DEV)
    for _ in range(3):
        oa, ga = _step(a, x, y)
    ent = [e for e in a._tape.plans.values() if e.get('state') == 'ready']
    assert ent, 'the third step did not replay a recorded list'
    ob, gb = _step(b, x, y)
    assert torch.equal(oa, ob)
    _same_grads(ga, gb)


def test_two_accumulating_steps_without_zero_grad():
    m = _seeded().set_compute_dtype('f32').to(DEV).train()
    (x1, y1), (x2, y2) = mc.blob_batch(2, 64, 12), mc.blob_batch(2, 64, 13)
    ref = _restated_grads(m, [x1, x2], [y1, y2])
    m.zero_grad()
    _step(m, x1.to(DEV), y1.to(DEV), zero=False)
    _, got = _step(m, x2.to(DEV), y2.to(DEV), zero=False)
    assert _cos(got, ref) > 0.9999
    gmax = max(float(v.abs().max()) for v in ref.values())
    for n in ref:
        if float(ref[n].abs().max()) > 1e-7 * gmax:
            rel = float((got[n].double().cpu() - ref[n]).norm() / (ref[n].norm() + 1e-30))
            assert rel <= 0.1, (n, rel)


# ---------------------------------------------------------------------------------------------------------------- 6. producer protocol
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_elu_serves_the_convolution_in_front_of_it(dtype, monkeypatch):
    # (gradients against float64 in fp32; a bf16 bias gradient is a cancelling sum of rounded terms, whose error scales with the
    # sum of their magnitudes, not with the result: the bf16 runs hold the logits and the launch list)
    m, calls = TC.check_probe_net('chain', DEV, monkeypatch, dtype=dtype, rtol=1e-4 if dtype == 'f32' else 3e-2,
                                  check_grads=dtype == 'f32')
    assert calls.count('segnb_elu_bwd') == 1
    assert calls.count('segnb_bn_act_bwd_reduce') == 0 and calls.count('segnb_bn_act_bwd_reduce_add') == 0


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_elu_falls_back_when_the_raw_output_has_a_second_consumer(dtype, monkeypatch):
    m, calls = TC.check_probe_net('second_consumer', DEV, monkeypatch, dtype=dtype, rtol=1e-4 if dtype == 'f32' else 3e-2,
                                  check_grads=dtype == 'f32')
    assert calls.count('segnb_elu_bwd') == 1 and calls.count('segnb_bn_act_bwd_reduce') == 1


# ---------------------------------------------------------------------------------------------------------------- 7. training
TRAIN_LR = 0.1


def test_64_bs8_bf16_sgd_training_loss_goes_down():
    """30 plain-SGD steps on one blob batch.  TRAIN_LR: the float64 restatement on the CPU meets the same condition with it
    (same seed and batch: mean of the first five losses 0.582, of the last five 0.380, falling at every step; 0.01 and 0.03
    meet it too, 0.601 -> 0.574 and 0.597 -> 0.530)."""
    from lib.losses import BCEWithLogitsLossAndSmoothJaccard
    from lib.models.squeezenet import SqueezeNet
    torch.manual_seed(0)
    m = SqueezeNet().to(DEV).train()
    x, y = mc.blob_batch(8, 64, 31)
    x, y = x.to(DEV), y.to(DEV)
    opt = torch.optim.SGD(m.parameters(), lr=TRAIN_LR)
    crit = BCEWithLogitsLossAndSmoothJaccard()
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = crit(m(x), y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(np.isfinite(losses)), losses
    assert all(torch.isfinite(p).all() for p in m.parameters())
    assert np.mean(losses[-5:]) < np.mean(losses[:5]), losses
