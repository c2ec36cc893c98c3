"""Derived bounds and exact probes for the convolutions that have an element-wise pass fused into them (helper module: no
fixtures, no pytest settings).  The launches run here, on 'cuda' through libsegnb_hip.so or on 'cpu' through a backend with the
call surface of the C ABI (oracle/abi_emulator.py or one of tests/fused_mutants.py); the references are float64, written from
include/segnb_hip.h (cited as H:<line>), not from a kernel.  tests/test_conv_fused_errbound_gpu.py and its CPU twin call the
check_* functions: each returns ({(family, dtype, tensor): worst err / bound}, [failure messages]).

1. Operands recomputed on load (H:506-518).  The consumer evaluates
       a  = round_bf16(drop * act((src - mean) * scale + shift))                                    SEGNB_TF_ACT    H:508
       dy = round_bf16(a * (dz - c1 - yhat * c2)),  dz = src * act'(z), yhat = (y - mean) * invstd  SEGNB_TF_BNBWD  H:511
   "in fp32 in a folded form: equal to the two-launch form up to fp32 rounding before the one bf16 rounding" (H:514-515); the
   folded forms are act(src * (scale * drop) + (shift - mean * scale) * drop) and a * (g * act') + (B * y + C) of
   csrc/bn_expr.h (bn_fold5_row).  The oracle evaluates the value in float64 and carries, with the X arithmetic of
   tests/ew_oracle.py, the bound e on what an fp32 chain adds -- the larger of the two forms' -- plus one more fp32 step for the
   negative side's multiplication.  A kernel's operand is round(v') with |v' - v| <= e and rounding is monotonic, so it lies
   between round(v - e) and round(v + e):
       slack = |round(act(t + e)) - round(act(t - e))|          (t: the value before the activation; act is monotonic)
   zero for almost every element, one bf16 step where the fp32 value may round either way.  A zero dropout multiplier makes
   every step of either chain exact: the operand is zero with zero slack.  An element of dy whose z lies within e of the kink
   carries |a * g| * (1 - act'-) in its e.  A convolution is linear in its operand, so
       bound(y) = errbound.bound_of(conv(operand), ...) + conv(slack, |w|)
   and the same for dx; for dW the widening is wgrad(slack_x, |dy|) + wgrad(|x|, slack_dy).  The share of elements with a
   non-zero slack is a CONDITION of the tests (at most ew_oracle.MAX_LEFT_OUT of an operand), asserted on the CPU.

2. The upsampled segment on the low-resolution tensor (H:580-587): the kernels multiply by four 2 x 2 phase matrices, each
   round_bf16 of the fp32 sum -- in ascending kernel position, as the masked pack jobs add them -- of the 3 x 3 taps it stands
   for; as one ConvTranspose2d(4, 2, 1) kernel, Wt[a][b] = sum_{kh in T[a], kw in T[b]} w[kh][kw] (segnb.engine.UpConvOp).  The
   skip segment and the 9-tap launches multiply by the taps rounded one by one.  The forward by segment rounds twice: "`out`
   holds the skip segment's convolution (+ bias) on entry" (H:583), a stored bf16 tensor, to which the second launch adds.

3. Activation epilogues (H:421-426): out = act(v), v = conv + bias or (conv + bias - mean) * scale + shift.  The steps after
   the K-term fp32 accumulation (errbound: K * 2^-23 * mag), each one fp32 operation of ew_oracle's arithmetic:
       H:422  conv + bias             counted as the (K + 1)-th term of the accumulation, as errbound.conv_refs does
       H:424  - mean, * scale, + shift   three steps; the accumulation's error is multiplied by |scale|
       H:426  act                     Lipschitz 1; LEAKY: one more multiplication
   A kernel may fold the affine part into acc * scale + ((bias - mean) * scale + shift) (three steps for the constant, two for
   the element): the bound carries the larger of the two chains.  Then bound = r_out |ref| (1 + 2^-8) + e (1 + r_out) + 2^-126.

4. Sums of a BatchNorm-reduce epilogue (H:435-441) are taken over dz = round(g * act'(z)) of the STORED data gradient g: they
   are held to float64 sums of that dz (ew_oracle.Oracle.dz_of) under P * 2^-23 * magnitude + 2^-126, P the pixel count -- the
   rule of test_conv_within_derived_bound for the forward statistics -- plus 2 |g| for every element dz_of finds at the kink.
"""
import torch
import torch.nn.functional as F

import errbound as eb
import ew_oracle as eo
from ew_oracle import X, add, mul, sub
from oracle import abi_emulator
from segnb import _native as nv
from segnb import convplan as cp
from segnb.engine import ConvOp, PackTable, Runtime, UpCatConvOp, View

U, TINY = eb.U_ACC, eb.TINY
EMU = abi_emulator.AbiEmulator()
SLOPE = 0.01

THIN_SHAPES = [(3, 9, 11, 48, 16, 2), (2, 17, 23, 72, 12, 1), (2, 33, 17, 200, 8, 2), (2, 24, 40, 112, 16, 1)]
# fprop_thin.hip thin_geometry serves N * H * W >= 4096 pixels only: the smallest odd shapes past that gate, 16 channels of dy
# and 12 padded to 16 (at 8, conv_c8_kernel takes the plain launch and only the fused one reaches conv_thin_kernel)
THIN_SERVED = [(2, 43, 48, 48, 16, 2), (3, 37, 37, 56, 12, 1)]
TF_SHAPES = [(2, 40, 56, 32, 1), (3, 33, 47, 24, 2)]
UPCAT_SHAPES = [(3, 12, 24, 12, 20), (2, 20, 16, 24, 32), (2, 20, 64, 64, 64), (2, 36, 128, 64, 64), (3, 36, 64, 32, 32)]
UPCAT_FORMS = ('virtual forward', 'virtual wgrad', 'forward by segment', 'segmented dgrad', 'upsum dgrad')


def sid(s):
    return 'x'.join(map(str, s))


class backend(object):
    """'cuda': the library.  'cpu': the emulator (or a mutant of it) as segnb._native's backend for the duration of the block"""

    def __init__(self, device, emu=None):
        self.device, self.emu = device, emu or EMU

    def __enter__(self):
        if self.device == 'cpu':
            nv.set_backend_for_testing(self.emu)

    def __exit__(self, *a):
        if self.device == 'cpu':
            nv.set_backend_for_testing(None)
        else:
            torch.cuda.synchronize()


def bf(t):
    return t.bfloat16().float()


def _nhwc_view(rt, t_nchw, Cp):
    v = View.alloc(rt, t_nchw.shape[0], t_nchw.shape[2], t_nchw.shape[3], Cp)
    v.dense()[..., :t_nchw.shape[1]] = t_nchw.permute(0, 2, 3, 1).to(rt.device, rt.tdtype)
    return v


def _pix_view(rt, t_nhwc):
    v = View.alloc(rt, *t_nhwc.shape)
    v.dense().copy_(t_nhwc.to(rt.device, rt.tdtype))
    return v


def _out(v):
    return v.dense().float().cpu()


def _sums(t):
    return t.sum(0).cpu()


# ------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------
def within(name, got, ref64, bound):
    """-> (worst err / bound, failure message or None); a NaN is a failure"""
    assert tuple(got.shape) == tuple(ref64.shape) == tuple(bound.shape), (name, got.shape, ref64.shape, bound.shape)
    ratio = (got.detach().double().cpu() - ref64).abs() / bound
    bad = ~(ratio <= 1.0)
    worst = float(torch.nan_to_num(ratio, nan=float('inf')).max()) if ratio.numel() else 0.0
    if not bool(bad.any()):
        return worst, None
    return worst, '%s: %d/%d elements over the bound, worst err/bound %.3g, first bad idx %s' % (
        name, int(bad.sum()), bad.numel(), worst, bad.nonzero()[:4].tolist())


def dw_bound(ref64, widening=None):
    """the f32 row of test_hip_ops.check(): 2e-4 of the tensor's largest magnitude + 2e-4 of the element (+ the slack term)"""
    b = 2e-4 * max(float(ref64.abs().max()), 1e-6) + 2e-4 * ref64.abs()
    return b if widening is None else b + widening


def refs_with_slack(x, sx, w, b, dy, sdy):
    """float64 y, dx, dW of the 3 x 3 / pad 1 convolution on the oracle operands x, dy [NCHW] and their bounds widened by the
    operands' slack (sx, sdy: tensors or None)"""
    r = eb.conv_refs(x, w, b, dy, 1, 1, False)
    zx, zdy = torch.zeros_like(x), torch.zeros_like(dy)
    sx, sdy = (zx if sx is None else sx), (zdy if sdy is None else sdy)
    wy, wdx, _ = eb._three(sx, w.abs(), None, sdy, 1, 1, False)
    _, _, wa = eb._three(sx, w, None, dy.abs(), 1, 1, False)
    _, _, wb = eb._three(x.abs(), w, None, sdy, 1, 1, False)
    r['bound_y'] = eb.bound_of(r['y'], r['mag_y'], r['K_y'], 'bf16') + wy
    r['bound_dx'] = eb.bound_of(r['dx'], r['mag_dx'], r['K_dx'], 'bf16') + wdx
    r['bound_dW'] = dw_bound(r['dW'], wa + wb)
    return r


def stats_check(name, st, y_stored):
    """[2][C] statistics against float64 sums of the stored y [N,H,W,C] -> ({tensor: ratio}, messages)"""
    P = y_stored.shape[0] * y_stored.shape[1] * y_stored.shape[2]
    v = y_stored.double().reshape(P, -1)
    return _sum_rows(name, st, P, ((v.sum(0), v.abs().sum(0), 0.0), ((v * v).sum(0), (v * v).sum(0), 0.0)), ('sum', 'sumsq'))


def _sum_rows(name, st, P, rows, tensors):
    ratios, msgs = {}, []
    for i, ((tot, mag, extra), tensor) in enumerate(zip(rows, tensors)):
        rat = (st[i].double()[:tot.shape[0]] - tot).abs() / (P * U * mag + extra + TINY)
        ratios[tensor] = float(torch.nan_to_num(rat, nan=float('inf')).max())
        bad = ~(rat <= 1.0)
        if bool(bad.any()):
            msgs.append('%s %s of the epilogue: %d/%d channels over P * 2^-23 * magnitude, worst ratio %.3g, first %s' % (
                name, tensor, int(bad.sum()), bad.numel(), ratios[tensor], bad.nonzero()[:4].flatten().tolist()))
    return ratios, msgs


def reduce_sums_check(name, sums, g_stored, y1, coef, act, slope):
    """the BatchNorm-reduce epilogue's [2][C] sums against float64 sums of dz = round(g * act'(z)) derived from the STORED data
    gradient g [N,H,W,C] (section 4); y1 [N,H,W,C] bf16 values, coef [4][C] fp32"""
    N, H, W, C = g_stored.shape
    orc = eo.Oracle()
    yk, ck = y1.bfloat16().contiguous(), coef.float().contiguous()
    co = orc.coefs(ck.data_ptr(), C)
    Y, d, amb = orc.dz_of('bf16', yk.data_ptr(), C, N, H, W, C, co, act, slope, None, None, None, 0, g=X(g_stored))
    D = eo.rnd(d.v, 'bf16').reshape(-1, C)
    kink = (2 * g_stored.double().abs() * amb).reshape(-1, C)
    yh = ((Y.v - co[2].v) * co[3].v).reshape(-1, C)
    rows = ((D.sum(0), D.abs().sum(0), kink.sum(0)), ((D * yh).sum(0), (D * yh).abs().sum(0), (kink * yh.abs()).sum(0)))
    return _sum_rows(name, sums, N * H * W, rows, ('sum dz', 'sum dz*yhat'))


# ------------------------------------------------------------------------------------------------------
# 1. the operand oracle
# ------------------------------------------------------------------------------------------------------
def _neg(act, slope):
    return {nv.ACT_RELU: 0.0, nv.ACT_LEAKY: eo._f32(slope), nv.ACT_NONE: 1.0}[act]


def _act64(t, neg):
    return torch.where(t > 0, t, t * neg)


def _rounded(v, e, neg):
    """v, e before the activation -> (round_bf16(act(v)), slack)"""
    r = lambda t: eb.round_out(_act64(t, neg), 'bf16').double()
    return r(v), (r(v + e) - r(v - e)).abs()


def tf_act_operand(src, coef, act, slope, drop):
    """src [N,H,W,C] bf16 values, coef [4][C] fp32, drop [N][C] fp32 or None -> (operand, slack) float64 [N,H,W,C]"""
    Y = X(src)
    sc, sh, mu = (X(coef[i].double()) for i in range(3))
    dm = X(torch.ones(1, 1, 1, 1) if drop is None else drop.double()[:, None, None, :])
    t1 = mul(add(mul(sub(Y, mu), sc), sh), dm)           # drop >= 0: drop * act(z) = act(drop * z) for these activations
    t2 = add(mul(Y, mul(sc, dm)), mul(sub(sh, mul(mu, sc)), dm))
    e = torch.maximum(t1.e, t2.e)
    e = torch.where(e > 0, e + U * (t1.v.abs() + e), e)    # the negative side's multiplication
    if act == nv.ACT_LEAKY:                                # ... which is inexact on its own: slope is no power of two
        n = t1.v * _neg(act, slope)
        e = e + U * n.abs() * ((t1.v < 0) & (n.float().double() != n))
    return _rounded(t1.v, e, _neg(act, slope))


def tf_bnbwd_operand(g, y, coef, bcoef, act, slope):
    """g, y [N,H,W,C] bf16 values, coef [4][C], bcoef [3][C] fp32 -> (operand dy, slack) float64"""
    G, Y = X(g), X(y)
    sc, sh, mu, isd = (X(coef[i].double()) for i in range(4))
    a, c1, c2 = (X(bcoef[i].double()) for i in range(3))
    z, zf = add(mul(sub(Y, mu), sc), sh), add(mul(Y, sc), sub(sh, mul(mu, sc)))
    ez = torch.maximum(z.e, zf.e)
    neg = _neg(act, slope)
    kink = (z.v.abs() <= ez) & (ez > 0) & (G.v != 0)
    dz = mul(G, X(torch.where(z.v > 0, torch.ones_like(z.v), torch.full_like(z.v, neg))))
    d1 = mul(a, sub(sub(dz, c1), mul(mul(sub(Y, mu), isd), c2)))
    B, C = mul(mul(X(-a.v), c2), isd), mul(a, sub(mul(mul(c2, isd), mu), c1))
    d2 = add(mul(a, dz), add(mul(B, Y), C))
    e = torch.maximum(d1.e, d2.e) + kink * (a.v * G.v).abs() * (1 - neg)
    return _rounded(d1.v, e, 1.0)


def slack_share(slack):
    return float((slack != 0).double().mean())


# ------------------------------------------------------------------------------------------------------
# 2a. the thin data gradient (conv_thin_kernel, fprop_thin.hip) and its BatchNorm-reduce epilogue
# ------------------------------------------------------------------------------------------------------
def thin_data(shape):
    N, H, W, C1, C2, act = shape
    gen = torch.Generator().manual_seed(H * 5 + C1)
    d = dict(w=bf(torch.randn(C2, C1, 3, 3, generator=gen) * (2.0 / (C1 * 9)) ** 0.5), dy=bf(torch.randn(N, C2, H, W, generator=gen)),
             y1=bf(torch.randn(N, H, W, C1, generator=gen)))
    d['coef'] = torch.stack([0.5 + torch.rand(C1, generator=gen), 0.3 * torch.randn(C1, generator=gen),
                             0.2 * torch.randn(C1, generator=gen), 0.5 + torch.rand(C1, generator=gen)]).contiguous()
    return d


def run_thin(device, shape, d, dy=None, fused=True, emu=None, census=None):
    """-> dx of the plain launch, dx of the fused launch, its sums [2][C1] (the last two None without `fused`)"""
    N, H, W, C1, C2, act = shape
    with backend(device, emu):
        rt = Runtime(device, 'bf16')
        op = ConvOp(rt, d['w'].to(device), None, [(C1, C1)], 1, 1, False, True)
        op.pack(H, W)
        dyv = _nhwc_view(rt, d['dy'] if dy is None else dy, op.Cop)
        g_plain, g_f = View.alloc(rt, N, H, W, C1), View.alloc(rt, N, H, W, C1)
        g_plain.t.fill_(3.0)
        g_f.t.fill_(5.0)
        if census is not None:
            census.take()
        op.dgrad(dyv, g_plain)
        if census is not None:
            census.seen = census.take()
        if not fused:
            return _out(g_plain), None, None
        assert op.dgrad_bnreduce_ok(dyv, g_f), 'the BatchNorm-reduce epilogue is not served at a dense layer\'s data gradient'
        y1, coef, sums = _pix_view(rt, d['y1']), d['coef'].to(device), rt.zeros((16, 2, C1), torch.float64)
        op.dgrad(dyv, g_f, bn_reduce=(y1, coef, sums, act, SLOPE))
        if census is not None:
            census.seen_fused = census.take()
    return _out(g_plain), _out(g_f), _sums(sums)


def _dgrad_ref(w, dy, C1):
    N, _, H, W = dy.shape
    z = torch.zeros(N, C1, H, W)
    _, dx, _ = eb._three(z, w, None, dy, 1, 1, False)
    _, mag, _ = eb._three(z, w.abs(), None, dy.abs(), 1, 1, False)
    return dx, mag


def check_thin(device, shape, emu=None, census=None):
    N, H, W, C1, C2, act = shape
    name, d = 'thin ' + sid(shape), thin_data(shape)
    dx_p, dx_f, sums = run_thin(device, shape, d, emu=emu, census=census)
    ref, mag = _dgrad_ref(d['w'], d['dy'], C1)
    ratios, msgs = {}, []
    for tag, dx in (('dx', dx_p), ('dx fused', dx_f)):
        r, m = within('%s %s' % (name, tag), dx.permute(0, 3, 1, 2), ref, eb.bound_of(ref, mag, C2 * 9, 'bf16'))
        ratios[('thin dgrad', 'bf16', tag)] = r
        msgs.append(m)
    msgs.append(eb.mismatches(name + ': the fused launch against the plain one', dx_f, dx_p))
    rs, ms = reduce_sums_check(name, sums, dx_f, d['y1'], d['coef'], act, SLOPE)
    ratios.update({('thin dgrad', 'bf16', k): v for k, v in rs.items()})
    return ratios, [m for m in msgs + ms if m]


def check_thin_impulses(device, shape, emu=None):
    """the plain impulse probes of test_conv_impulses_exact_fprop_dgrad: dy zero but for impulses at least 3 apart"""
    N, H, W, C1, C2, act = shape
    d, msgs = thin_data(shape), []
    for pas in range(eb.impulse_passes(N, C2, H, W, 3)):
        dy = eb.impulse_tensor(N, C2, H, W, 3, pas)
        dx, _, _ = run_thin(device, shape, d, dy=dy, fused=False, emu=emu)
        want = eb.impulse_expect_dx(torch.zeros(N, C1, H, W), d['w'], dy, 1, 1, False, 'bf16')
        msgs.append(eb.mismatches('thin %s dx pass %d' % (sid(shape), pas), dx.permute(0, 3, 1, 2), want))
    return {}, [m for m in msgs if m]


# ------------------------------------------------------------------------------------------------------
# 2b. consumer-side BatchNorm (segnb_conv_fprop_tf, segnb_conv_wgrad_tf)
# ------------------------------------------------------------------------------------------------------
def _coef(gen, C, sep):
    """scale 0.5 .. 1.5; shift and mean of opposite signs, alternating by channel: |shift - mean * scale| >= 0.5 + 0.2 * 0.5
    in every channel with `sep`, so that a transformed zero is far from zero; invstd 0.5 .. 1.5"""
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
    if sep:
        shift, mean = sign * (0.5 + 0.3 * torch.rand(C, generator=gen)), -sign * (0.2 + 0.2 * torch.rand(C, generator=gen))
    else:
        shift, mean = 0.3 * torch.randn(C, generator=gen), 0.2 * torch.randn(C, generator=gen)
    return torch.stack([0.5 + torch.rand(C, generator=gen), shift, mean, 0.5 + torch.rand(C, generator=gen)]).contiguous()


def tf_data(shape, use_drop):
    """the operands of a layer C1 = 32 -> C2 whose input is act(BatchNorm(y0)) and whose dy is the BatchNorm-backward apply of
    (g, y), with the oracle operands A, DY [NCHW] and their slack"""
    N, H, W, C2, act = shape
    C1, C2p = 32, cp.pad8(C2)
    gen = torch.Generator().manual_seed(H * 3 + C2 + 7 * int(use_drop))
    d = dict(w=bf(torch.randn(C2, C1, 3, 3, generator=gen) * (2.0 / (C1 * 9)) ** 0.5), b=torch.randn(C2, generator=gen) * 0.1,
             y0=bf(torch.randn(N, H, W, C1, generator=gen)), y0b=bf(torch.randn(N, H, W, C1, generator=gen)),
             g=bf(torch.randn(N, H, W, C2p, generator=gen)), y=bf(torch.randn(N, H, W, C2p, generator=gen)),
             coef0=_coef(gen, C1, True), coef2=_coef(gen, C2p, False), slope=SLOPE, act=act)
    d['bcoef2'] = torch.stack([0.5 + torch.rand(C2p, generator=gen), 0.05 * torch.randn(C2p, generator=gen),
                               0.05 * torch.randn(C2p, generator=gen)]).contiguous()
    d['drop'] = (torch.rand(N, C1, generator=gen) > 0.3).float().mul(1.0 / 0.7).contiguous() if use_drop else None
    d['coef2'][:, C2:] = 0
    d['bcoef2'][:, C2:] = 0
    d['g'][..., C2:] = 0
    return tf_oracle(d, C2)


def tf_oracle(d, C2):
    A, sA = tf_act_operand(d['y0'], d['coef0'], d['act'], d['slope'], d['drop'])
    DY, sDY = tf_bnbwd_operand(d['g'], d['y'], d['coef2'], d['bcoef2'], d['act'], d['slope'])
    nchw = lambda t: t[..., :C2].permute(0, 3, 1, 2).contiguous()
    d.update(A=A.permute(0, 3, 1, 2).contiguous(), sA=sA.permute(0, 3, 1, 2).contiguous(), DY=nchw(DY), sDY=nchw(sDY),
             pad_dy=float(DY[..., C2:].abs().max()) if DY.shape[-1] > C2 else 0.0)
    return d


def run_tf(device, shape, d, emu=None, census=None, stats=True, reduce=True):
    """-> y, statistics [2][C2p], dx (None where the data gradient is not served), its reduce sums, dW with both transforms, with
    the input's alone (dy = the oracle operand, stored), with dy's alone (x = the oracle operand, stored)"""
    N, H, W, C2, act = shape
    C1 = 32
    out = {}
    with backend(device, emu):
        rt = Runtime(device, 'bf16')
        w = d['w'].to(device)
        op = ConvOp(rt, w, d['b'].to(device), [(C1, C1)], 1, 1, False, True)
        op.pack(H, W)
        C2p = op.Cop
        y0, y0b, gv, yv = (_pix_view(rt, d[k]) for k in ('y0', 'y0b', 'g', 'y'))
        coef0, coef2, bcoef2 = (d[k].to(device) for k in ('coef0', 'coef2', 'bcoef2'))
        drop = None if d['drop'] is None else d['drop'].to(device)
        tfx = ConvOp.tf_act(coef0, C1, act, d['slope'], drop)
        tfd = ConvOp.tf_bnbwd(yv, coef2, bcoef2, act, d['slope'])
        y2, st = View.alloc(rt, N, H, W, C2p), rt.zeros((16, 2, C2p), torch.float64)
        assert op.fprop_tf_ok(y0, y2) and op.wgrad_tf_ok(y0, gv)
        if census is not None:
            census.take()
        op.fprop_tf(y0, tfx, y2, st if stats else None)
        out['y'], out['stats'] = _out(y2), _sums(st)
        dx, sums = View.alloc(rt, N, H, W, C1), rt.zeros((16, 2, C1), torch.float64)
        served = op.dgrad_tf_ok(gv, dx)
        assert served == (C2 == 32), 'the data gradient on a recomputed dy is served at 32 output channels only'
        out['dx'] = out['sums'] = None
        if served:
            op.dgrad_tf(gv, tfd, dx, bn_reduce=(y0b, coef0, sums, act, d['slope']) if reduce else None)
            out['dx'], out['sums'] = _out(dx), _sums(sums)
        a_st, dy_st = _nhwc_view(rt, d['A'], C1), _nhwc_view(rt, d['DY'], C2p)
        p = op.plan(H, W)
        for key, xv, tx, dv, td in (('dW', y0, tfx, gv, tfd), ('dW x', y0, tfx, dy_st, None), ('dW dy', a_st, None, gv, tfd)):
            op.wgrad_tf(xv, tx, dv, td)
            gw = torch.zeros_like(w)
            nv.call('segnb_unpack_wgrad', nv.ptr(p['dwp'][0]), nv.ptr(gw), op.Cop, op.Cip, 9, op.s_out, op.s_in, p['tapoff_fwd'][0],
                    nv.ptr(op.out_map), nv.ptr(op.in_map), 1, rt.stream)
            if device != 'cpu':
                torch.cuda.synchronize()
            out[key] = gw.cpu()
        if census is not None:
            census.seen = census.take()
    return out


def check_tf(device, shape, use_drop, emu=None, d=None, census=None):
    N, H, W, C2, act = shape
    name = 'tf %s%s' % (sid(shape), ' drop' if use_drop else '')
    d = d or tf_data(shape, use_drop)
    o = run_tf(device, shape, d, emu=emu, census=census)
    r = refs_with_slack(d['A'], d['sA'], d['w'], d['b'], d['DY'], d['sDY'])
    fam, ratios, msgs = 'tf', {}, []

    def hold(tensor, got, ref, bound):
        ratios[(fam, 'bf16', tensor)], m = within('%s %s' % (name, tensor), got, ref, bound)
        msgs.append(m)
    hold('y', o['y'][..., :C2].permute(0, 3, 1, 2), r['y'], r['bound_y'])
    if o['y'].shape[-1] > C2 and float(o['y'][..., C2:].abs().max()) != 0.0:
        msgs.append(name + ' y: pad channels not zero')
    rs, ms = stats_check(name, o['stats'], o['y'])
    if o['dx'] is not None:
        hold('dx', o['dx'].permute(0, 3, 1, 2), r['dx'], r['bound_dx'])
        rs2, ms2 = reduce_sums_check(name, o['sums'], o['dx'], d['y0b'], d['coef0'], act, d['slope'])
        rs.update(rs2)
        ms += ms2
    ratios.update({(fam, 'bf16', k): v for k, v in rs.items()})
    _, _, wa = eb._three(d['sA'], d['w'], None, d['DY'].abs(), 1, 1, False)
    _, _, wb = eb._three(d['A'].abs(), d['w'], None, d['sDY'], 1, 1, False)
    hold('dW', o['dW'], r['dW'], r['bound_dW'])
    hold('dW x', o['dW x'], r['dW'], dw_bound(r['dW'], wa))
    hold('dW dy', o['dW dy'], r['dW'], dw_bound(r['dW'], wb))
    return ratios, [m for m in msgs + ms if m]


# ---- exact probes: coefficients that make the transforms exact
def tf_exact_data(shape, use_drop, x_src, g_src):
    """scale = 1, mean = shift = 0, slope 2^-6, dropout multipliers 0 / 1 / 2, a = 2, c1 = c2 = 0: a = drop * act(src) and
    dy = a * g * act'(y) exactly.  y holds -1, 0 and 1: act'(0) is the negative side's (H:485, csrc/bn_expr.h act_grad)"""
    N, H, W, C2, act = shape
    C1, C2p = 32, cp.pad8(C2)
    ones, zeros = lambda C: torch.ones(C), lambda C: torch.zeros(C)
    gen = torch.Generator().manual_seed(3 * H + C2)
    d = dict(w=bf(torch.randn(C2, C1, 3, 3, generator=gen) * (2.0 / (C1 * 9)) ** 0.5), b=torch.randn(C2, generator=gen) * 0.1,
             y0=x_src.permute(0, 2, 3, 1).contiguous(), y0b=torch.zeros(N, H, W, C1), slope=2.0 ** -6, act=act,
             coef0=torch.stack([ones(C1), zeros(C1), zeros(C1), ones(C1)]).contiguous(),
             coef2=torch.stack([ones(C2p), zeros(C2p), zeros(C2p), ones(C2p)]).contiguous(),
             bcoef2=torch.stack([2 * ones(C2p), zeros(C2p), zeros(C2p)]).contiguous())
    d['g'] = F.pad(g_src.permute(0, 2, 3, 1), (0, C2p - C2)).contiguous()
    d['y'] = (torch.randint(0, 3, (N, H, W, C2p), generator=gen) - 1).float()
    d['drop'] = torch.randint(0, 3, (N, C1), generator=gen).float().contiguous() if use_drop else None
    d['coef2'][:, C2:] = 0
    d['bcoef2'][:, C2:] = 0
    d = tf_oracle(d, C2)
    assert float(d['sA'].abs().max()) == 0.0 and float(d['sDY'].abs().max()) == 0.0, 'the probe operands are exact'
    return d


def signed(t, pas=0):
    """every other impulse negative"""
    idx = t.nonzero()
    s = t.clone()
    for i, ix in enumerate(idx.tolist()):
        if (i + pas) % 2:
            s[tuple(ix)] = -s[tuple(ix)]
    return s


def check_tf_impulses(device, shape, use_drop, emu=None, passes=range(9)):
    """fprop_tf and dgrad_tf on impulse operands of both signs (shifted_impulses: nine grids that cover every pixel): == the
    plain expectations on the transformed impulses"""
    N, H, W, C2, act = shape
    msgs = []
    for pas in passes:
        x, g = shifted_impulses(N, 32, H, W, 3, pas), shifted_impulses(N, C2, H, W, 3, pas)
        d = tf_exact_data(shape, use_drop, x, g)
        o = run_tf(device, shape, d, emu=emu, stats=False, reduce=False)
        name = 'tf %s pass %d' % (sid(shape), pas)
        msgs.append(eb.mismatches(name + ' y', o['y'][..., :C2].permute(0, 3, 1, 2),
                                  eb.impulse_expect_y(d['A'], d['w'], d['b'], 1, 1, False, 'bf16')))
        if o['dx'] is not None:
            msgs.append(eb.mismatches(name + ' dx', o['dx'].permute(0, 3, 1, 2),
                                      eb.impulse_expect_dx(d['A'], d['w'], d['DY'], 1, 1, False, 'bf16')))
    return {}, [m for m in msgs if m]


def check_tf_wgrad_probe(device, shape, use_drop, emu=None, max_passes=None):
    """wgrad_tf with one non-zero pixel per input channel (errbound.wgrad_probe_tensor, both signs) and a dense dy on an
    eighth-integer grid: every dW element is one exact product"""
    N, H, W, C2, act = shape
    msgs = []
    gen = torch.Generator().manual_seed(W + C2)
    g = torch.randint(-15, 16, (N, C2, H, W), generator=gen).float() / 8
    for pas in range(eb.wgrad_probe_passes(N, 32, H, W))[:max_passes]:
        d = tf_exact_data(shape, use_drop, signed(eb.wgrad_probe_tensor(N, 32, H, W, pas), pas), g)
        o = run_tf(device, shape, d, emu=emu, stats=False, reduce=False)
        want = eb.wgrad_expect(d['A'], d['w'], d['DY'], 1, 1, False)
        for key in ('dW', 'dW x', 'dW dy'):
            msgs.append(eb.mismatches('tf %s %s pass %d' % (sid(shape), key, pas), o[key], want))
    return {}, [m for m in msgs if m]


# ------------------------------------------------------------------------------------------------------
# 2c. virtual concat and the segmented forms of the decoder's first convolution
# ------------------------------------------------------------------------------------------------------
T = ((2,), (1, 2), (0, 1), (0,))           # segnb.engine.UpConvOp.T


def phase_weights(w_up, tap_rounded=False):
    """[Co][Cu][3][3] fp32 -> the ConvTranspose2d(4, 2, 1) kernel [Cu][Co][4][4] the up segment multiplies by: each entry
    round_bf16 of the fp32 sum, in ascending kernel position, of the 3 x 3 taps it stands for (float64 values)"""
    Co, Cu = w_up.shape[:2]
    wt = torch.zeros(Cu, Co, 4, 4, dtype=torch.float64)
    for a in range(4):
        for b in range(4):
            acc = torch.zeros(Co, Cu)
            for kh in T[a]:
                for kw in T[b]:
                    acc = acc + (bf(w_up[:, :, kh, kw]) if tap_rounded else w_up[:, :, kh, kw].float())
            wt[:, :, a, b] = bf(acc).double().t()
    return wt


def upcat_data(shape):
    N, S, Cu, Cs, Co = shape
    gen = torch.Generator().manual_seed(S * 131 + Cu + Co)
    Ci = Cu + Cs
    return dict(w=torch.randn(Co, Ci, 3, 3, generator=gen) * (2.0 / (Ci * 9)) ** 0.5, u=bf(torch.randn(N, Cu, S // 2, S // 2, generator=gen)),
                sk=bf(torch.randn(N, Cs, S, S, generator=gen)), dy=bf(torch.randn(N, Co, S, S, generator=gen)))


def upcat_op(rt, shape, w):
    N, S, Cu, Cs, Co = shape
    op = UpCatConvOp(rt, w, None, [(Cu, cp.pad8(Cu)), (Cs, cp.pad8(Cs))], need_dgrad=True)
    op.segment_wgrad = op.force_segmented = op.segment_fwd = True
    return op


def upcat_forms(device, shape, emu=None):
    """which forms the gates of UpCatConvOp serve at this shape (nothing is launched)"""
    N, S, Cu, Cs, Co = shape
    with backend(device, emu):
        rt = Runtime(device, 'bf16')
        op = upcat_op(rt, shape, torch.zeros(Co, Cu + Cs, 3, 3, device=device))
        op.virtual_concat, op.segment_wgrad = True, False
        virt = bool(op.virtual(N, S, S))
        op.virtual_concat, op.segment_wgrad = False, True
        op._seg.clear()
        fseg = bool(op.fwd_segmented(N, S, S, op.Cop))
        dseg = bool(op.segmented(N, S, S))
        op.force_segmented = False
        op._seg.clear()
        ups = bool(op.upsum(N, S, S))
    return {'virtual forward': virt, 'virtual wgrad': virt, 'forward by segment': fseg, 'segmented dgrad': dseg, 'upsum dgrad': ups}


def run_upcat(device, shape, d, emu=None, want=UPCAT_FORMS + ('plain', 'segmented wgrad')):
    """the launches of test_upcat_segmented_backward_vs_torch, each form where its gate serves the shape -> dict of CPU tensors
    (absent: not served or not wanted)"""
    N, S, Cu, Cs, Co = shape
    o = {}
    with backend(device, emu):
        rt = Runtime(device, 'bf16')
        wd = d['w'].to(device)
        op = upcat_op(rt, shape, wd)
        Cup, Csp = op.up_pad, op.sk_pad
        PackTable(rt, op.full.pack_jobs(S, S) + op.skip.pack_jobs(S, S) + op.up.pack_jobs(S // 2, S // 2),
                  'segnb_pack_weight_multi', 'segnb_pack_weight').run()
        cat = View.alloc(rt, N, S, S, Cup + Csp)
        cat.dense()[..., :Cu] = F.interpolate(d['u'], scale_factor=2, mode='nearest').permute(0, 2, 3, 1).to(device, torch.bfloat16)
        cat.dense()[..., Cup:Cup + Cs] = d['sk'].permute(0, 2, 3, 1).to(device, torch.bfloat16)
        uv, dyv = _nhwc_view(rt, d['u'], Cup), _nhwc_view(rt, d['dy'], op.Cop)
        duv = View.alloc(rt, N, S // 2, S // 2, Cup)
        duv.t.fill_(7.0)                                   # every element must be overwritten
        if 'plain' in want:
            yv = View.alloc(rt, N, S, S, op.Cop)
            op.fprop(cat, yv)                              # (no low-resolution tensor bound yet: the one 9-tap launch)
            o['y plain'] = _out(yv)
        op.bind_up(uv, duv)
        cat_noup = View.alloc(rt, N, S, S, Cup + Csp)      # the upsampled copy is NOT read below: leave it as garbage
        cat_noup.t.fill_(5.0)
        cat_noup.dense()[..., Cup:] = cat.dense()[..., Cup:]
        op.virtual_concat, op.segment_wgrad = True, False
        op._seg.clear()
        if op.virtual(N, S, S) and ('virtual forward' in want or 'virtual wgrad' in want):
            yvirt, vstats = View.alloc(rt, N, S, S, op.Cop), rt.zeros((16, 2, op.Cop), torch.float64)
            yvirt.t.fill_(3.0)
            op.fprop(cat_noup, yvirt, vstats)
            gwv = torch.zeros_like(wd)
            op.wgrad(cat_noup, dyv, gwv, unpack=False)
            PackTable(rt, op.full.unpack_jobs(S, S, gwv), 'segnb_unpack_wgrad_multi', 'segnb_unpack_wgrad').run()
            o['y virtual'], o['stats virtual'], o['dW virtual'] = _out(yvirt), _sums(vstats), gwv.cpu()
        op.virtual_concat, op.segment_wgrad = False, True
        op._seg.clear()
        if op.fwd_segmented(N, S, S, op.Cop) and 'forward by segment' in want:
            yseg, stats = View.alloc(rt, N, S, S, op.Cop), rt.zeros((16, 2, op.Cop), torch.float64)
            yseg.t.fill_(3.0)
            op.fprop(cat_noup, yseg, stats)
            o['y segment'], o['stats segment'] = _out(yseg), _sums(stats)
        if 'segmented dgrad' in want:
            assert op.segmented(N, S, S)
            dcat = View.alloc(rt, N, S, S, Cup + Csp)
            op.dgrad(dyv, dcat)
            o['dskip'], o['du'] = _out(dcat)[..., Cup:Cup + Cs], _out(duv)
        op.force_segmented = False
        op._seg.clear()
        if op.upsum(N, S, S) and 'upsum dgrad' in want:
            dcat_s, duv_s = View.alloc(rt, N, S, S, Cup + Csp), View.alloc(rt, N, S // 2, S // 2, Cup)
            dcat_s.t.fill_(9.0)
            duv_s.t.fill_(7.0)
            op.bind_up(uv, duv_s)
            assert op.writes_du(N, S, S) and not op.segmented(N, S, S)
            op.dgrad(dyv, dcat_s)
            op.bind_up(uv, duv)
            dfull = View.alloc(rt, N, S, S, Cup + Csp)
            op.full.dgrad(dyv, dfull)
            o['dskip upsum'], o['du upsum'], o['dcat upsum'], o['dfull'] = (_out(dcat_s)[..., Cup:Cup + Cs], _out(duv_s), _out(dcat_s),
                                                                           _out(dfull))
        op.force_segmented = True
        op._seg.clear()
        if 'segmented wgrad' in want:
            gw = torch.zeros_like(wd)
            op.wgrad(cat, dyv, gw, unpack=False)
            PackTable(rt, op.unpack_jobs(S, S, gw), 'segnb_unpack_wgrad_multi', 'segnb_unpack_wgrad').run()
            o['dW segment'] = gw.cpu()
    o['Cup'] = Cup
    return o


def upcat_refs(shape, d):
    """float64 references and bounds.  'tap': conv2d(cat(interpolate(u), skip)) with the taps rounded one by one (the 9-tap
    launches, the skip segment); 'seg': the up segment through the phase weights (section 2)"""
    N, S, Cu, Cs, Co = shape
    w, u, sk, dy = d['w'], d['u'].double(), d['sk'].double(), d['dy'].double()
    wr = bf(w).double()
    up = lambda t: F.interpolate(t, scale_factor=2, mode='nearest')
    K_y, K_dx = (Cu + Cs) * 9 + 1, Co * 9
    r = {}
    y, dcat, dW = eb._three(torch.cat([up(u), sk], 1), wr, None, dy, 1, 1, False)
    mag_y, mag_dcat, _ = eb._three(torch.cat([up(u), sk], 1).abs(), wr.abs(), None, dy.abs(), 1, 1, False)
    r['y tap'], r['bound y tap'] = y, eb.bound_of(y, mag_y, K_y, 'bf16')
    r['dskip'], r['bound dskip'] = dcat[:, Cu:], eb.bound_of(dcat[:, Cu:], mag_dcat[:, Cu:], K_dx, 'bf16')
    r['dW'], r['bound dW'] = dW, dw_bound(dW)
    # du of the plain launch's slice, summed 2 x 2 AFTER its bf16 store (H:566-568): four stored values, one more rounding
    pool = lambda t: F.avg_pool2d(t, 2) * 4
    r['du tap'] = pool(dcat[:, :Cu])
    per = eb.bound_of(dcat[:, :Cu], mag_dcat[:, :Cu], K_dx, 'bf16')
    r['bound du tap'] = eb.R_BF16 * r['du tap'].abs() * (1 + eb.R_BF16) + (pool(per) + 4 * U * pool(dcat[:, :Cu].abs())) * (1 + eb.R_BF16) + TINY
    # the segmented forms
    wt = phase_weights(w[:, :Cu])
    us = u.clone().requires_grad_(True)
    yu = F.conv_transpose2d(us, wt, None, stride=2, padding=1)
    yu.backward(dy)
    ys = F.conv2d(sk, wr[:, Cu:], None, padding=1)
    mag_u = F.conv_transpose2d(u.abs(), wt.abs(), None, stride=2, padding=1)
    mag_s = F.conv2d(sk.abs(), wr[:, Cu:].abs(), None, padding=1)
    r['y seg'] = ys + yu.detach()
    stored_skip = eb.bound_of(ys, mag_s, Cs * 9 + 1, 'bf16')                 # the first launch's stored result (H:583)
    r['bound y seg'] = stored_skip + eb.bound_of(r['y seg'], mag_u + ys.abs() + stored_skip, Cu * 4 + 1, 'bf16')
    r['du seg'] = us.grad
    r['bound du seg'] = eb.bound_of(us.grad, _du_mag(dy, wt), Co * 16, 'bf16')
    return r


def _du_mag(dy, wt):
    us = torch.zeros(dy.shape[0], wt.shape[0], dy.shape[2] // 2, dy.shape[3] // 2, dtype=torch.float64, requires_grad=True)
    F.conv_transpose2d(us, wt.abs(), None, stride=2, padding=1).backward(dy.abs())
    return us.grad


def check_upcat(device, shape, emu=None):
    N, S, Cu, Cs, Co = shape
    name, d = 'upcat ' + sid(shape), upcat_data(shape)
    o, r = run_upcat(device, shape, d, emu=emu), upcat_refs(shape, d)
    Cup = o['Cup']
    ratios, msgs = {}, []
    nchw = lambda t, C: t[..., :C].permute(0, 3, 1, 2)

    def hold(fam, tensor, got, ref, bound):
        ratios[(fam, 'bf16', tensor)], m = within('%s %s %s' % (name, fam, tensor), got, ref, bound)
        msgs.append(m)

    def pads(tag, t, C):
        if t.shape[-1] > C and float(t[..., C:].abs().max()) != 0.0:
            msgs.append('%s %s: pad channels not zero' % (name, tag))

    def stats(fam, st, y):
        rs, ms = stats_check('%s %s' % (name, fam), st, y)
        ratios.update({(fam, 'bf16', k): v for k, v in rs.items()})
        msgs.extend(ms)
    hold('plain concat', 'y', nchw(o['y plain'], Co), r['y tap'], r['bound y tap'])
    if 'y virtual' in o:
        hold('virtual forward', 'y', nchw(o['y virtual'], Co), r['y tap'], r['bound y tap'])
        msgs.append(eb.mismatches(name + ': the virtual forward against the launch over the materialised concat',
                                  o['y virtual'][..., :Co], o['y plain'][..., :Co]))
        pads('y virtual', o['y virtual'], Co)
        stats('virtual forward', o['stats virtual'], o['y virtual'])
        hold('virtual wgrad', 'dW', o['dW virtual'], r['dW'], r['bound dW'])
    if 'y segment' in o:
        hold('forward by segment', 'y', nchw(o['y segment'], Co), r['y seg'], r['bound y seg'])
        pads('y segment', o['y segment'], Co)
        stats('forward by segment', o['stats segment'], o['y segment'])
    hold('segmented dgrad', 'dskip', o['dskip'].permute(0, 3, 1, 2), r['dskip'], r['bound dskip'])
    hold('segmented dgrad', 'du', nchw(o['du'], Cu), r['du seg'], r['bound du seg'])
    pads('du', o['du'], Cu)
    hold('segmented wgrad', 'dW', o['dW segment'], r['dW'], r['bound dW'])
    if 'du upsum' in o:
        hold('upsum dgrad', 'dskip', o['dskip upsum'].permute(0, 3, 1, 2), r['dskip'], r['bound dskip'])
        hold('upsum dgrad', 'du', nchw(o['du upsum'], Cu), r['du tap'], r['bound du tap'])
        if float((o['dcat upsum'][..., :Cup] - 9.0).abs().max()) != 0.0:
            msgs.append(name + ': the high-resolution slice is not to be written')
        # = the plain data gradient's stored slice, summed 2 x 2 in fp32 and rounded once
        f = o['dfull'][..., :Cup]
        ref = bf(((f[:, 0::2, 0::2] + f[:, 0::2, 1::2]) + f[:, 1::2, 0::2]) + f[:, 1::2, 1::2])
        msgs.append(eb.mismatches(name + ': du of the fused upsum against the 2 x 2 fp32 sum of the stored slice', o['du upsum'], ref))
        msgs.append(eb.mismatches(name + ': d skip of the fused upsum against the plain launch', o['dcat upsum'][..., Cup:],
                                  o['dfull'][..., Cup:]))
    return ratios, [m for m in msgs if m]


# ---- exact probes
def shifted_impulses(N, C, H, W, k, pas):
    """errbound.impulse_tensor's construction on a grid shifted by (pas % k, pas // k % k): impulses 2^j (both signs) at least k
    apart, one channel at a time; over k * k passes the grids cover every pixel, so both sides of every seam and, on the
    low-resolution tensor, even and odd high-resolution rows and columns next to it"""
    oy, ox = pas % k, (pas // k) % k
    rows, cols = list(range(oy, H, k)), list(range(ox, W, k))
    t = torch.zeros(N, C, H, W)
    P = N * len(rows) * len(cols)
    i = 0
    for n in range(N):
        for r in rows:
            for c in cols:
                t[n, (i + pas * P) % C, r, c] = 2.0 ** ((i + pas) % 5 - 2) * (-1) ** (i + pas)
                i += 1
    return t


def grid_weights(shape):
    """weights on a 1/64 grid below 1/2: the sum of the up to four products behind one output of a 9-tap launch over a 2 x 2
    block of the upsampled tensor is exact in fp32 in every order"""
    N, S, Cu, Cs, Co = shape
    gen = torch.Generator().manual_seed(S + Cu)
    w = torch.randint(-31, 32, (Co, Cu + Cs, 3, 3), generator=gen).float() / 64
    return torch.where(w == 0, torch.full_like(w, 1.0 / 64), w)


def _exact32(t):
    assert torch.equal(t.float().double(), t), 'the expectation must be exact in fp32'
    return t.float()


def check_upcat_impulses(device, shape, emu=None, passes=None):
    """virtual concat: impulses on u (3 apart on the LOW-resolution grid: the 2 x 2 blocks they become are then one to a 3 x 3
    window) and on the skip tensor, grid weights: y == the float64 convolution; dW with a dense dy on an eighth-integer grid.
    Forward by segment (real weights, impulses on u 2 apart: one product per output): y == u * the rounded phase weight.
    Segmented data gradient (dy impulses 4 apart: one product per element of du, 3 apart would do for d skip)."""
    N, S, Cu, Cs, Co = shape
    forms = upcat_forms(device, shape, emu)
    msgs, name = [], 'upcat ' + sid(shape)
    up = lambda t: F.interpolate(t, scale_factor=2, mode='nearest')
    gen = torch.Generator().manual_seed(S + Co)
    dense_dy = torch.randint(-15, 16, (N, Co, S, S), generator=gen).float() / 8
    real = upcat_data(shape)['w']
    wt = phase_weights(real[:, :Cu])
    zero_u, zero_sk = torch.zeros(N, Cu, S // 2, S // 2), torch.zeros(N, Cs, S, S)
    for pas in (range(16) if passes is None else passes):
        if forms['virtual forward'] and pas < 9:
            d = dict(w=grid_weights(shape), u=shifted_impulses(N, Cu, S // 2, S // 2, 3, pas), sk=shifted_impulses(N, Cs, S, S, 3, pas),
                     dy=dense_dy)
            o = run_upcat(device, shape, d, emu=emu, want=('virtual forward', 'virtual wgrad'))
            y, _, dW = eb._three(torch.cat([up(d['u']), d['sk']], 1), d['w'], None, d['dy'], 1, 1, False)
            msgs.append(eb.mismatches('%s virtual y pass %d' % (name, pas), o['y virtual'][..., :Co].permute(0, 3, 1, 2), bf(_exact32(y))))
            msgs.append(eb.mismatches('%s virtual dW pass %d' % (name, pas), o['dW virtual'], _exact32(dW)))
        if forms['forward by segment'] and pas < 4:
            d = dict(w=real, u=shifted_impulses(N, Cu, S // 2, S // 2, 2, pas), sk=zero_sk, dy=dense_dy)
            o = run_upcat(device, shape, d, emu=emu, want=('forward by segment',))
            want = F.conv_transpose2d(d['u'].double(), wt, None, stride=2, padding=1)
            msgs.append(eb.mismatches('%s segment y pass %d' % (name, pas), o['y segment'][..., :Co].permute(0, 3, 1, 2), bf(_exact32(want))))
        d = dict(w=real, u=zero_u, sk=zero_sk, dy=shifted_impulses(N, Co, S, S, 4, pas))
        o = run_upcat(device, shape, d, emu=emu, want=('segmented dgrad',))
        us = zero_u.double().requires_grad_(True)
        F.conv_transpose2d(us, wt, None, stride=2, padding=1).backward(d['dy'].double())
        msgs.append(eb.mismatches('%s du pass %d' % (name, pas), o['du'][..., :Cu].permute(0, 3, 1, 2), bf(_exact32(us.grad))))
        want = eb.impulse_expect_dx(zero_sk, bf(real[:, Cu:]), d['dy'], 1, 1, False, 'bf16')
        msgs.append(eb.mismatches('%s d skip pass %d' % (name, pas), o['dskip'].permute(0, 3, 1, 2), want))
        if len([m for m in msgs if m]) >= 4:
            break
    return {}, [m for m in msgs if m]


# ------------------------------------------------------------------------------------------------------
# 2d. activation epilogues (segnb_conv_fprop_act, segnb_upconv_fprop_act)
# ------------------------------------------------------------------------------------------------------
def act_data(case, dtype):
    """the data recipe of test_conv_fprop_act_epilogue"""
    name, N, H, W, segs, Co, k, s, p, transposed = case
    Ci = sum(r for r, _ in segs)
    gen = torch.Generator().manual_seed(len(name) * 7 + Co)
    q = bf if dtype == 'bf16' else (lambda t: t)
    d = dict(w=q(torch.randn(Co, Ci, k, k, generator=gen) * (2.0 / (Ci * k * k)) ** 0.5), b=torch.randn(Co, generator=gen) * 0.1,
             x=q(torch.randn(N, Ci, H, W, generator=gen)))
    d['act'], d['slope'] = (nv.ACT_LEAKY, SLOPE) if 'leaky' in name or k == 2 else (nv.ACT_RELU, 0.0)
    d['gamma'], d['beta'] = 0.5 + torch.rand(Co, generator=gen), 0.2 * torch.randn(Co, generator=gen)
    d['rm'], d['rv'] = 0.1 * torch.randn(Co, generator=gen), 0.5 + torch.rand(Co, generator=gen)
    if transposed:
        d['w'] = q(torch.randn(Ci, Co, k, k, generator=gen) * (2.0 / (Ci * k * k)) ** 0.5)
    return d


def run_act(device, case, dtype, with_bn, d, emu=None):
    """-> y [N,Ho,Wo,Cop], the wider buffer around it, coef [4][Cop] as the launch read it (or None); (None, None, None) where
    the kernel has no such form (the one-launch transposed convolution takes no folded BatchNorm)"""
    name, N, H, W, segs, Co, k, s, p, transposed = case
    with backend(device, emu):
        r = Runtime(device, dtype)
        op = ConvOp(r, d['w'].to(device), d['b'].to(device), segs, s, p, transposed, need_dgrad=False)
        op.pack(H, W)
        Ho, Wo = op.out_hw(H, W)
        xv = View.alloc(r, N, H, W, op.Cip)
        off, roff = 0, 0
        for real, padded in segs:
            xv.dense()[..., off:off + real] = d['x'][:, roff:roff + real].permute(0, 2, 3, 1).to(device, r.tdtype)
            off += padded
            roff += real
        buf = r.zeros((N, Ho, Wo, op.Cop + 16))
        yv = View(buf, N, Ho, Wo, op.Cop, op.Cop + 16, 8)
        coef = None
        if with_bn:
            coef = r.zeros((4, op.Cop), torch.float32)
            stats = r.zeros((16, 2, op.Cop), torch.float64)
            rm, rv, gam, bet = (d[key].to(device) for key in ('rm', 'rv', 'gamma', 'beta'))          # (kept alive)
            nv.call('segnb_bn_finalize', nv.ptr(stats), Co, op.Cop, float(N * Ho * Wo), nv.ptr(gam), nv.ptr(bet), 1e-5, 0.1,
                    nv.ptr(rm), nv.ptr(rv), None, 0, nv.ptr(coef), r.stream)
            if device != 'cpu':
                torch.cuda.synchronize()
        if 'upconv' in name:
            if with_bn:
                assert not op.act_epilogue_ok(H, W, N, yv.ld, coef)     # (no folded BatchNorm on that kernel)
                return None, None, None
            assert op.act_epilogue_ok(H, W, N, yv.ld, coef)
        else:
            assert op.act_epilogue_ok(H, W)
        op.fprop(xv, yv, None, epilogue=(coef, d['act'], d['slope']))
        if device != 'cpu':
            torch.cuda.synchronize()
        return yv.dense().float().cpu(), buf.float().cpu(), None if coef is None else coef.cpu()


def act_ref(case, dtype, d, coef):
    """-> float64 reference and bound of section 3"""
    name, N, H, W, segs, Co, k, s, p, transposed = case
    Ci = sum(r for r, _ in segs)
    x, w = d['x'].double(), d['w'].double()
    conv = eb._conv64(x, w, None, s, p, transposed)
    mag = eb._conv64(x.abs(), w.abs(), d['b'].double().abs(), s, p, transposed)
    K = Ci * k * k + 1
    ch = lambda t: X(t.double()[None, :, None, None])
    acc = X(conv + d['b'].double()[None, :, None, None], K * U * mag)
    if coef is None:
        v = acc
    else:
        sc, sh, mu = (ch(coef[i, :Co]) for i in range(3))
        v = add(mul(sub(acc, mu), sc), sh)
        vf = add(mul(X(conv, K * U * mag), sc), add(mul(sub(ch(d['b']), mu), sc), sh))
        v = X(v.v, torch.maximum(v.e, vf.e))
    neg = _neg(d['act'], d['slope'])
    ref = _act64(v.v, neg)
    e = v.e + (U * (ref.abs() + v.e) if d['act'] == nv.ACT_LEAKY else 0.0)
    return ref, eb.bound_of(ref, e / U, 1, dtype)


def check_act(device, case, dtype, with_bn, emu=None):
    name, N, H, W, segs, Co, k, s, p, transposed = case
    d = act_data(case, dtype)
    y, buf, coef = run_act(device, case, dtype, with_bn, d, emu=emu)
    if y is None:
        return {}, []
    ref, bound = act_ref(case, dtype, d, coef)
    fam = 'act epilogue' + (' upconv' if 'upconv' in name else '') + (' evalbn' if with_bn else '')
    ratio, m = within('%s [%s] y' % (name, dtype), y[..., :Co].permute(0, 3, 1, 2), ref, bound)
    msgs = [m]
    if float(buf[..., :8].abs().max()) != 0.0 or float(buf[..., 8 + y.shape[-1]:].abs().max()) != 0.0:
        msgs.append(name + ': written outside the channel slice')
    if y.shape[-1] > Co and float(y[..., Co:].abs().max()) != 0.0:
        msgs.append(name + ': padding channels must stay zero')
    return {(fam, dtype, 'y'): ratio}, [m for m in msgs if m]
