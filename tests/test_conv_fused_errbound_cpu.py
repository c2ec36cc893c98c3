"""The instrument of tests/test_conv_fused_errbound_gpu.py proved on the CPU (tests/fused_errbound.py): the same cases through the
ABI emulator pass every bound and every `==`; the operand oracle's slack admits an fp32 evaluation of either form and stays
under the 1 % cap; the probe operands cover what they claim and leave one product per element; and each mutant of
tests/fused_mutants.py -- the emulator wrong in one place -- fails at least one of the checks."""
import pytest
import torch
import torch.nn.functional as F

import errbound as eb
import ew_oracle as eo
import fused_errbound as fe
import fused_mutants as fm
from segnb import _native as nv
from test_hip_ops import ACT_EP_CASES

ACT_RUNS = [(c, bn, dt) for c in ACT_EP_CASES for bn in (False, True) for dt in ('f32', 'bf16') if dt == 'bf16' or 'upconv' not in c[0]]


def _ok(res):
    ratios, msgs = res
    assert not msgs, '\n'.join(msgs)
    return ratios


# ------------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize('shape', fe.THIN_SHAPES + fe.THIN_SERVED, ids=fe.sid)
def test_thin_on_the_emulator(shape):
    _ok(fe.check_thin('cpu', shape))
    _ok(fe.check_thin_impulses('cpu', shape))


@pytest.mark.parametrize('use_drop', [False, True], ids=['nodrop', 'drop'])
@pytest.mark.parametrize('shape', fe.TF_SHAPES, ids=fe.sid)
def test_tf_on_the_emulator(shape, use_drop):
    d = fe.tf_data(shape, use_drop)
    # the condition of the widened bound: at most 1 % of an operand may round either way
    for key in ('sA', 'sDY'):
        share = fe.slack_share(d[key])
        print('%s %s: %.4f %% of the elements carry slack' % (fe.sid(shape), key, 100 * share))
        assert share <= eo.MAX_LEFT_OUT
    shh = (d['coef0'][1] - d['coef0'][2] * d['coef0'][0]).abs()
    assert float(shh.min()) >= 0.3                                  # a transformed zero is far from zero in every channel
    if use_drop:
        off = (d['drop'] == 0)[:, :, None, None].expand_as(d['A'])
        assert bool(off.any()) and float(d['A'][off].abs().max()) == 0.0 and float(d['sA'][off].abs().max()) == 0.0
    assert d['pad_dy'] == 0.0
    _ok(fe.check_tf('cpu', shape, use_drop, d=d))
    _ok(fe.check_tf_impulses('cpu', shape, use_drop))
    _ok(fe.check_tf_wgrad_probe('cpu', shape, use_drop))


@pytest.mark.parametrize('shape', fe.UPCAT_SHAPES, ids=fe.sid)
def test_upcat_on_the_emulator(shape):
    _ok(fe.check_upcat('cpu', shape))
    _ok(fe.check_upcat_impulses('cpu', shape))


@pytest.mark.parametrize('case,with_bn,dtype', ACT_RUNS, ids=['%s|%s|%s' % (c[0], 'evalbn' if bn else 'act', dt) for c, bn, dt in ACT_RUNS])
def test_act_epilogue_on_the_emulator(case, with_bn, dtype):
    _ok(fe.check_act('cpu', case, dtype, with_bn))


# ------------------------------------------------------------------------------------------------------ the constructions
@pytest.mark.parametrize('act', [nv.ACT_RELU, nv.ACT_LEAKY], ids=['relu', 'leaky'])
def test_slack_admits_fp32_in_either_form(act):
    """the 33 x 47, 32-channel recipe: an fp32 evaluation of the two-launch form and of the folded form (csrc/bn_expr.h) rounds
    to the oracle's operand or to a neighbour inside the slack, element by element"""
    shape = (3, 33, 47, 32, act)
    d = fe.tf_data(shape, True)
    y, co, dm = d['y0'], d['coef0'], d['drop'][:, None, None, :]
    neg = 0.0 if act == nv.ACT_RELU else float(torch.tensor(fe.SLOPE, dtype=torch.float32))
    a32 = lambda t: torch.where(t > 0, t, t * neg)
    forms = {'two-launch': a32((y - co[2]) * co[0] + co[1]) * dm, 'folded': a32(y * (co[0] * dm) + (co[1] - co[2] * co[0]) * dm)}
    A, sA = d['A'].permute(0, 2, 3, 1), d['sA'].permute(0, 2, 3, 1)
    for tag, v in forms.items():
        diff = (fe.bf(v).double() - A).abs()
        print('TF_ACT %s: %.2e of the elements flip, none outside the slack' % (tag, float((diff > 0).double().mean())))
        assert bool((diff <= sA).all()), int((diff > sA).sum())
    g, yy, c2, bc = d['g'], d['y'], d['coef2'], d['bcoef2']
    sel = torch.where((yy - c2[2]) * c2[0] + c2[1] > 0, 1.0, neg)
    B, C = -bc[0] * bc[2] * c2[3], bc[0] * (bc[2] * c2[3] * c2[2] - bc[1])
    forms = {'two-launch': bc[0] * (g * sel - bc[1] - (yy - c2[2]) * c2[3] * bc[2]), 'folded': bc[0] * (g * sel) + (B * yy + C)}
    C2 = d['DY'].shape[1]
    DY, sDY = d['DY'].permute(0, 2, 3, 1), d['sDY'].permute(0, 2, 3, 1)
    for tag, v in forms.items():
        diff = (fe.bf(v)[..., :C2].double() - DY).abs()
        print('TF_BNBWD %s: %.2e of the elements flip, none outside the slack' % (tag, float((diff > 0).double().mean())))
        assert bool((diff <= sDY).all()), int((diff > sDY).sum())
    assert fe.slack_share(d['sA']) <= eo.MAX_LEFT_OUT and fe.slack_share(d['sDY']) <= eo.MAX_LEFT_OUT


def test_phase_weights_are_the_upsampled_convolution():
    """ConvTranspose2d(4, 2, 1) with the summed taps IS conv3x3(pad 1) of the nearest x 2 upsample (weights on a grid: every sum
    exact), and rounding after the sum differs from summing rounded taps on real weights -- what mutant (d) gets wrong"""
    shape = (2, 12, 8, 8, 8)
    w = fe.grid_weights(shape)[:, :8]
    u = torch.randint(-7, 8, (2, 8, 6, 6)).double()
    a = F.conv_transpose2d(u, fe.phase_weights(w), None, stride=2, padding=1)
    b = F.conv2d(F.interpolate(u, scale_factor=2, mode='nearest'), w.double(), None, padding=1)
    assert torch.equal(a, b)
    real = fe.upcat_data((3, 12, 24, 12, 20))['w'][:, :24]
    assert not torch.equal(fe.phase_weights(real), fe.phase_weights(real, tap_rounded=True))


@pytest.mark.parametrize('shape', fe.UPCAT_SHAPES, ids=fe.sid)
def test_upcat_probes_cover_every_pixel_with_one_product(shape):
    N, S, Cu, Cs, Co = shape
    h = S // 2
    every = lambda n, hh, ww: {(i, r, c) for i in range(n) for r in range(hh) for c in range(ww)}
    px = lambda t: set(map(tuple, (t != 0).sum(1).nonzero().tolist()))
    ones = lambda *s: torch.ones(*s, dtype=torch.float64)
    placed_u, placed_sk, placed_u2, placed_dy = set(), set(), set(), set()
    chan_u = torch.zeros(Cu, dtype=torch.bool)
    for pas in range(9):
        u, sk = fe.shifted_impulses(N, Cu, h, h, 3, pas), fe.shifted_impulses(N, Cs, S, S, 3, pas)
        cat = torch.cat([F.interpolate(u, scale_factor=2, mode='nearest'), sk], 1)
        # a 3 x 3 window holds the 2 x 2 block of at most one u pixel (<= 4 products, exact on the weight grid) or one skip impulse
        per_u = F.conv2d((u != 0).sum(1, keepdim=True).double(), ones(1, 1, 2, 2), padding=1)
        assert float(per_u.max()) <= 1 and float(F.conv2d((sk != 0).sum(1, keepdim=True).double(), ones(1, 1, 3, 3), padding=1).max()) <= 1
        assert float(F.conv2d((cat != 0).double(), ones(1, Cu + Cs, 3, 3), padding=1).max()) <= 5
        placed_u |= px(u)
        placed_sk |= px(sk)
        chan_u |= (u != 0).sum((0, 2, 3)) > 0
    for pas in range(4):
        u = fe.shifted_impulses(N, Cu, h, h, 2, pas)
        assert float(F.conv_transpose2d((u != 0).sum(1, keepdim=True).double(), ones(1, 1, 4, 4), stride=2, padding=1).max()) <= 1
        placed_u2 |= px(u)
    for pas in range(16):
        dy = fe.shifted_impulses(N, Co, S, S, 4, pas)
        ind = (dy != 0).sum(1, keepdim=True).double()
        us = torch.zeros(N, 1, h, h, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(us, ones(1, 1, 4, 4), stride=2, padding=1).backward(ind)
        assert float(us.grad.max()) <= 1 and float(F.conv2d(ind, ones(1, 1, 3, 3), padding=1).max()) <= 1
        placed_dy |= px(dy)
    # every pixel: the first and the last image, both sides of every seam errbound.essential_pixels names, and on u the even
    # and the odd high-resolution rows and columns next to them
    assert placed_u == every(N, h, h) == placed_u2 and placed_sk == every(N, S, S) == placed_dy
    assert set(eb.essential_pixels(N, S, S)) <= placed_sk and set(eb.essential_pixels(N, h, h)) <= placed_u
    assert bool(chan_u.all())


@pytest.mark.parametrize('shape', fe.TF_SHAPES, ids=fe.sid)
def test_tf_probes_cover_the_seams_with_one_product(shape):
    N, H, W, C2, act = shape
    placed = set()
    for pas in range(9):
        x, g = fe.shifted_impulses(N, 32, H, W, 3, pas), fe.shifted_impulses(N, C2, H, W, 3, pas)
        my, mdx, _ = eb.products_per_element(x, g, (C2, 32, 3, 3), 1, 1, False)
        assert my <= 1 and mdx <= 1
        assert bool((x < 0).any() and (x > 0).any())
        placed |= set(map(tuple, (x != 0).sum(1).nonzero().tolist()))
    assert placed == {(n, r, c) for n in range(N) for r in range(H) for c in range(W)} >= set(eb.essential_pixels(N, H, W))
    placed = set()
    for pas in range(eb.wgrad_probe_passes(N, 32, H, W)):
        x = fe.signed(eb.wgrad_probe_tensor(N, 32, H, W, pas), pas)
        assert bool(((x != 0).sum((0, 2, 3)) == 1).all())
        assert eb.products_per_element(x, torch.ones(N, C2, H, W), (C2, 32, 3, 3), 1, 1, False)[2] <= 1
        placed |= set(map(tuple, (x != 0).sum(1).nonzero().tolist()))
    assert set(eb.essential_pixels(N, H, W)) <= placed
    assert {(0, 0, 0), (N - 1, H - 1, W - 1), (0, H - 1, 0), (N - 1, 0, W - 1)} <= placed


# ------------------------------------------------------------------------------------------------------ the mutants
ACT_1X1 = [c for c in ACT_EP_CASES if c[0] == 'general 1x1 40->24'][0]
KILLERS = {
    'a tf_pad_transformed': lambda m: fe.check_tf('cpu', fe.TF_SHAPES[0], False, emu=m),
    'b folded_shift_no_drop': lambda m: fe.check_tf('cpu', fe.TF_SHAPES[0], True, emu=m),
    'c upcat_seam_row': lambda m: fe.check_upcat('cpu', fe.UPCAT_SHAPES[0], emu=m),
    'd phase_tap_rounded': lambda m: fe.check_upcat_impulses('cpu', fe.UPCAT_SHAPES[0], emu=m, passes=range(2)),
    'e upsum_bf16': lambda m: fe.check_upcat('cpu', fe.UPCAT_SHAPES[1], emu=m),
    'f thin_drop_tap': lambda m: fe.check_thin('cpu', fe.THIN_SHAPES[0], emu=m),
    'g evalbn_before_bias': lambda m: fe.check_act('cpu', ACT_1X1, 'bf16', True, emu=m),
    'h actgrad_ge': lambda m: fe.check_tf_impulses('cpu', fe.TF_SHAPES[0], False, emu=m, passes=range(1)),
}


@pytest.mark.parametrize('flag', sorted(fm.MUTANTS))
def test_each_mutant_fails_a_check(flag):
    ratios, msgs = KILLERS[flag](fm.MUTANTS[flag]())
    worst = max(ratios.values()) if ratios else float('nan')
    print('mutant %s: %d failures, the worst element at %.3g times its bound\n  %s' % (flag, len(msgs), worst, '\n  '.join(msgs[:4])))
    assert msgs, 'the mutant passed'
    _ok(KILLERS[flag](None))                                        # ... and the unmodified emulator passes the same check
