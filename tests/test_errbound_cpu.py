"""The instrument of tests/test_conv_errbound_gpu.py proved on the CPU (tests/errbound.py): the derived bound admits correct
fp32-accumulating arithmetic at every geometry of the case table, flags a kernel that ignores one weight wherever a tolerance can
see that at all, and the impulse operands really leave one product per output element -- which is what catches the same defect at
the deep-K shapes, where no tolerance can."""
import pytest
import torch
import torch.nn.functional as F

import errbound as eb
from test_hip_ops import CONV_CASES, DEEPK_CASES, DMA_CASES, RW_CASES, _run_conv, on_emulator

IDS = [c[0] for c in CONV_CASES]
EMU_CASES = [c for c in CONV_CASES if c[0] in ('3x3 concat pad', '7x7 s2 stem', '1x1 s2', 'roll 3x3 p0 co24', '3x3 deep K cat',
                                               'convT 3x3 s2 p0', 'convT 4x4 s2 upf co24')]
ALL_SHAPES = CONV_CASES + [eb.full_case(c) for c in DMA_CASES + RW_CASES]


def _conv32(x, w, b, case):
    name, N, H, W, segs, Co, k, s, p, transposed = case
    if transposed:
        return F.conv_transpose2d(x, w, b, stride=s, padding=p)
    return F.conv2d(x, w, b, stride=s, padding=p)


def _fp32_then_bf16(case, w, b, x, dy):
    """what a correct bf16 kernel computes, in torch's own fp32 summation order: y and dx rounded to bf16"""
    xr = x.clone().requires_grad_(True)
    y = _conv32(xr, w, b, case)
    y.backward(dy)
    return y.detach().bfloat16().float(), xr.grad.bfloat16().float()


@pytest.mark.parametrize('case', CONV_CASES, ids=IDS)
def test_bound_admits_fp32_accumulation(case):
    name, N, H, W, segs, Co, k, s, p, transposed = case
    w, b, x, dy = eb.operands(case, 'bf16')
    r = eb.conv_refs(x, w, b, dy, s, p, transposed)
    assert r['K_y'] == sum(q for q, _ in segs) * k * k + 1 and r['K_dx'] == Co * k * k
    y, dx = _fp32_then_bf16(case, w, b, x, dy)
    ry = eb.assert_within_bound(name + ' y', y, r['y'], r['mag_y'], r['K_y'], 'bf16')
    rdx = eb.assert_within_bound(name + ' dx', dx, r['dx'], r['mag_dx'], r['K_dx'], 'bf16')
    print('%s: worst err/bound y %.3f dx %.3f' % (name, ry, rdx))


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('case', EMU_CASES, ids=[c[0] for c in EMU_CASES])
def test_bound_admits_the_abi_emulator(case, dtype):
    name, N, H, W, segs, Co, k, s, p, transposed = case
    w, b, x, dy = eb.operands(case, dtype)
    r = eb.conv_refs(x, w, b, dy, s, p, transposed)
    with on_emulator():
        y, st, dx, gw, _, _ = _run_conv('cpu', dtype, case, w, b, x, dy)
    eb.assert_within_bound(name + ' y', y[..., :Co].permute(0, 3, 1, 2), r['y'], r['mag_y'], r['K_y'], dtype)
    dxr, pads = eb.real_channels(dx, segs)
    eb.assert_within_bound(name + ' dx', dxr, r['dx'], r['mag_dx'], r['K_dx'], dtype)
    assert pads == 0.0 and (y.shape[-1] == Co or float(y[..., Co:].abs().max()) == 0.0)


def _mutant(w):
    m = w.clone()
    m[0, 0, 0, 0] = 0.0
    assert float(w[0, 0, 0, 0]) != 0.0
    return m


@pytest.mark.parametrize('case', CONV_CASES, ids=IDS)
def test_bound_flags_a_kernel_that_ignores_one_weight(case):
    """w[0,0,0,0] zeroed on the side under test only.  Everywhere but at the deep shapes the bound must see it; at the deep
    shapes K * 2^-23 * mag alone exceeds one product -- the hole that the impulse probes close (next test).  Which side a table
    entry falls on is decided by its term count, not by its name.  Not seen (K * terms * 2^-23 >= 1): '3x3 deep K' (K = 9361,
    no element flagged), '3x3 deep K cat' (9289, one outlier among 324 outputs) and '3x3 deep 7x7' (4609, not in DEEPK_CASES
    but just as deep).  Must be seen: every other entry, among them '1x1 deep K' (K = 2305, as '3x3 wide'), whose lost
    product the bound still catches at 12 outputs."""
    name, N, H, W, segs, Co, k, s, p, transposed = case
    w, b, x, dy = eb.operands(case, 'bf16')
    r = eb.conv_refs(x, w, b, dy, s, p, transposed)
    y, dx = _fp32_then_bf16(case, _mutant(w), b, x, dy)
    flagged = int((eb.bound_ratio(y, r['y'], r['mag_y'], r['K_y'], 'bf16') > 1).sum())
    flagged_dx = int((eb.bound_ratio(dx, r['dx'], r['mag_dx'], r['K_dx'], 'bf16') > 1).sum())
    print('%s: mutant flagged at %d elements of y, %d of dx' % (name, flagged, flagged_dx))
    # One product is about |x||w|, mag about `terms` of them, so the bound's floor K * 2^-23 * mag is about K * terms * 2^-23
    # products: where that is below 1 (K = terms < 2^11.5 = 2896) the loss must show; above, the floor hides a typical product.
    # (a transposed convolution of stride s sums ceil(k / s)^2 taps per channel into an output, not the k^2 that K_y counts)
    terms = sum(q for q, _ in segs) * (-(-k // s)) ** 2 + 1 if transposed else r['K_y']
    if terms * r['K_y'] * eb.U_ACC < 1.0:
        assert case not in DEEPK_CASES or name == '1x1 deep K'          # (K = 2305: still visible)
        assert flagged > 0
    else:
        # the hole that the impulse probes close: nothing but a stray outlier among the N * Ho * Wo outputs that lost a product
        assert flagged <= 0.01 * y.shape[0] * y.shape[2] * y.shape[3], flagged
        if name == '3x3 deep K':
            assert flagged == 0
    assert flagged_dx > 0           # (K_dx = Co * k * k is small at every shape of the table)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('case', DEEPK_CASES, ids=[c[0] for c in DEEPK_CASES])
def test_impulse_probe_catches_the_mutant_at_deep_k(case, dtype):
    name, N, H, W, segs, Co, k, s, p, transposed = case
    Ci = sum(q for q, _ in segs)
    w, b, _, dy = eb.operands(case, dtype)
    caught = 0
    for pas in range(eb.impulse_passes(N, Ci, H, W, k)):
        x = eb.impulse_tensor(N, Ci, H, W, k, pas)
        want = eb.impulse_expect_y(x, w, b, s, p, transposed, dtype)
        with on_emulator():
            y_ok = _run_conv('cpu', dtype, case, w, b, x, dy)[0]
            y_mut = _run_conv('cpu', dtype, case, _mutant(w), b, x, dy)[0]
        assert eb.mismatches(name, y_ok[..., :Co].permute(0, 3, 1, 2), want) is None      # exact on the unmutated emulator
        caught += eb.mismatches(name, y_mut[..., :Co].permute(0, 3, 1, 2), want) is not None
    assert caught >= 1          # the pass(es) in which channel 0 carries an impulse under tap (0, 0)


@pytest.mark.parametrize('case', ALL_SHAPES, ids=[c[0] for c in ALL_SHAPES])
def test_impulse_operands_leave_one_product_per_element(case):
    """a condition of the exact tests: no element of y, dx or dW receives more than one non-zero product; every real channel
    carries an impulse in some pass; the image borders carry impulses"""
    name, N, H, W, segs, Co, k, s, p, transposed = case
    Ci = sum(q for q, _ in segs)
    Ho, Wo = eb.out_size(case)
    wshape = (Ci, Co, k, k) if transposed else (Co, Ci, k, k)
    npass = max(eb.impulse_passes(N, Ci, H, W, k), eb.impulse_passes(N, Co, Ho, Wo, k))
    used_x, used_dy = torch.zeros(Ci, dtype=torch.bool), torch.zeros(Co, dtype=torch.bool)
    for pas in range(npass):
        x, dy = eb.impulse_tensor(N, Ci, H, W, k, pas), eb.impulse_tensor(N, Co, Ho, Wo, k, pas)
        my, mdx, _ = eb.products_per_element(x, dy, wshape, s, p, transposed)
        assert my <= 1 and mdx <= 1, (pas, my, mdx)
        used_x |= (x != 0).sum((0, 2, 3)) > 0
        used_dy |= (dy != 0).sum((0, 2, 3)) > 0
        for t in (x, dy):
            on = (t != 0).sum(1) > 0            # [N, H, W]
            assert bool(on[:, 0, 0].all() and on[:, -1, -1].all() and on[:, 0, -1].all() and on[:, -1, 0].all())
    assert bool(used_x.all()) and bool(used_dy.all())
    if name == '3x3 deep K':
        assert eb.impulse_passes(N, Ci, H, W, k) == 4
    dense = torch.ones(N, Co, Ho, Wo)
    placed = set()
    for pas in range(eb.wgrad_probe_passes(N, Ci, H, W)):
        x = eb.wgrad_probe_tensor(N, Ci, H, W, pas)
        assert bool(((x != 0).sum((0, 2, 3)) == 1).all())
        assert eb.products_per_element(x, dense, wshape, s, p, transposed)[2] <= 1
        placed |= set(map(tuple, (x != 0).sum(1).nonzero().tolist()))
    # coverage of the pixels actually placed over all passes, however few the channels
    assert set(eb.essential_pixels(N, H, W)) <= placed
    assert {(0, 0, 0), (N - 1, H - 1, W - 1), (0, H - 1, 0), (N - 1, 0, W - 1)} <= placed                 # corners, first / last image
    assert N == 1 or {n for n, _, _ in placed} >= {0, 1, N - 1}
    lin = {(n * H + r) * W + c for n, r, c in placed}
    for step in (64, 256):
        assert N * H * W <= step or (step - 1 in lin and step in lin)                                   # both sides of a pixel-tile seam
    if W > 16:
        c0 = 16 * ((W - 1) // 16)
        assert {(N - 1, H - 1, c0 - 1), (N - 1, H - 1, c0)} <= placed                                     # the last row's ragged segment
        assert any((n, r, 16) in placed for n, r, c in placed if c == 15)                               # both sides of a strip seam
    if H > 8:
        assert any((n, 8, c) in placed for n, r, c in placed if r == 7)                                 # both sides of a row seam
