"""A float64 oracle of the loss and metric entry points with derived per-element bounds (helper module: no fixtures, no
pytest settings).

Written from the mathematics and from the contracts in include/segnb_hip.h ("Per-pixel binary losses and metrics",
segnb_absmax_f32, segnb_pr_histogram) and include/segnb_mc_loss.h -- not from a kernel and not from oracle/abi_emulator.py.

  binary      ls = logsigmoid(x), p = exp(ls), e = -t ls + log1p(p) (the double-sigmoid BCE element, t = float(label), any
              integer), de = (1 - p)(p / (1 + p) - t), pt = exp(-e), f = (1 - pt)^gamma e, df = (gamma (1 - pt)^(gamma - 1) pt e
              + (1 - pt)^gamma) de; the seven sums, the finalize and dlogits of the header
  multi       logp = log_softmax(x) (mode 0) or x (mode 1), p = exp(logp), the sums S[3C + 8], fin[8 + 3C] and dlogits of
              segnb_mc_loss.h
  histogram   bucket = number of thresholds strictly below sigmoid(x), per class of the target (0 / non-zero)
  absmax      max |x|; a NaN anywhere surfaces as NaN

Values carry their bound as ew_oracle.X does (v float64, e a bound on |an fp32 chain - v|), with ew_oracle's add / sub / mul / div
and four more operations, the libm functions.  For a function f that is monotonic on the interval [v - e_in, v + e_in],

    e_out = max |f(v +- e_in) - f(v)| + L * U_ACC * |f| + 2^-126

which is |f'(v)| e_in + L U_ACC |f(v)| where the interval is short, and stays a bound where it is not (pow near 0, exp of a
large argument).  L is the ulp charge of the device's libm function: twice the worst ulp error measured on the MI355X against
numpy float64 over the argument ranges the cases reach, rounded up (profiles/loss_oracle_ratios.txt holds the measurements;
nothing was tuned on a loss kernel's output).  2^-126 covers results below the smallest normal fp32.

The bound charges magnitudes, not one formulation: 1 - p, 1 - pt, p / (1 + p) - t and (x - max) - log(sum) are charged
U_ACC * max(|a|, |b|) (`sub_m`), so `1.f - p` and a sigmoid(-x) both fit.  The log-softmax is charged on x - max and log(sum),
not on |x|: it is shift invariant (x - (max + log sum) rounds the log-sum-exp at the magnitude of the logits and does not fit
under a common offset).  A sum of exponentials over C
classes is additionally charged (C - 1)(L_EXP + 2) U_ACC of its value: an online max / rescale pass multiplies the running sum
by one more exp per class.

pt == 1.  The focal derivative at pt == 1 is its limit: 0 for gamma > 0 (-1 times d(e) for gamma == 0).  (1 - pt)^(gamma - 1)
with gamma < 1 is unbounded at 0; an fp32 1 - pt is either 0 -- then the term is the limit, 0 -- or at least 2^-24, so the
operation `powq` bounds it by the values at 2^-24 and at the interval's upper end, and by the term's own magnitude.

Sums.  Integers (sum t, counts, T_c) are exact.  A real sum is bounded by the sum of its elements' bounds plus
K_ACC32 * U_ACC * sum |v_i|: a wave's worth (64) of sequential fp32 additions before a float64 accumulator takes over.  The
finalize runs in float64 on the oracle sums with the sums' bounds pushed through the same operations, and is rounded once to fp32.
"""
import os

import numpy as np
import torch

import errbound as eb
import ew_oracle as eo
from ew_oracle import X, add, sub, mul, div

U, TINY = eb.U_ACC, eb.TINY
# ulp charges of the device libm (fp32), 2 x the worst measured, rounded up: profiles/loss_oracle_ratios.txt
L_EXP, L_LOG, L_LOG1P, L_POW = 2, 4, 2, 3
K_ACC32 = 64
OM_MIN = 2.0 ** -24                      # the smallest non-zero fp32 value of 1 - pt, pt in [0.5, 1)
MAX_AMBIGUOUS = 0.01
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'loss_oracle_ratios.txt')
F64 = torch.float64


def c_(v):
    return X(torch.tensor(float(v), dtype=F64))


def f32(v):
    return float(np.float32(v))


def neg(a):
    return X(-a.v, a.e)


def mono(a, fn, L, lo=None, hi=None):
    """a monotonic libm function of a value with a bound; lo / hi: what the argument cannot leave in any implementation"""
    v = fn(a.v)
    al, ah = a.v - a.e, a.v + a.e
    if lo is not None:
        al = al.clamp(min=lo)
    if hi is not None:
        ah = ah.clamp(max=hi)
    prop = torch.maximum((fn(ah) - v).abs(), (fn(al) - v).abs())
    return X(v, prop + L * U * (v.abs() + prop) + TINY)


def sub_m(a, b):
    """a - b charged on the operands' magnitude, not on the (possibly cancelled) result"""
    prop = a.e + b.e
    return X(a.v - b.v, prop + U * (torch.maximum(a.v.abs(), b.v.abs()) + prop))


def powq(om, q):
    """om^q for om = 1 - pt in [0, 1]; q < 0: see the module docstring (0 at om == 0: the limit of the term it belongs to)"""
    if q == 0:
        return X(torch.ones_like(om.v))
    if q == 1:
        return om
    if q > 0:
        return mono(om, lambda b: b.clamp(min=0.0) ** q, L_POW, lo=0.0)
    lo, hi = (om.v - om.e), (om.v + om.e).clamp(min=OM_MIN)
    v = torch.where(om.v > 0, om.v.clamp(min=1e-300) ** q, torch.zeros_like(om.v))
    prop = torch.maximum((hi ** q - v).abs(), (lo.clamp(min=OM_MIN) ** q - v).abs())
    prop = torch.where(lo <= 0, torch.maximum(prop, v.abs()), prop)
    return X(v, prop + L_POW * U * (v.abs() + prop) + TINY)


def dsum(x, dim=None):
    """the sum of fp32 elements: each one's bound, and K_ACC32 fp32 additions' worth of rounding on the magnitudes"""
    if dim is None:
        return X(x.v.sum(), x.e.sum() + K_ACC32 * U * x.v.abs().sum())
    return X(x.v.sum(dim), x.e.sum(dim) + K_ACC32 * U * x.v.abs().sum(dim))


def out_bound(x):
    """the bound of an fp32 output"""
    return eb.bound_of(x.v, x.e / U, 1, 'f32')


def ratio(got, x):
    """worst |got - v| / bound over an output (a NaN or an infinity in `got` counts as infinite)"""
    got = torch.as_tensor(got).detach().double().cpu().reshape(x.v.shape)
    r = (got - x.v).abs() / out_bound(x)
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float('inf')))
    return float(torch.nan_to_num(r, nan=float('inf')).max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------------ binary
class Spec(object):
    """segnb_loss_spec with its floats as the fp32 numbers the library receives"""
    FIELDS = ('w_bce', 'w_focal', 'w_jaccard', 'w_sjaccard', 'w_dice', 'smooth', 'eps', 'norm', 'focal_mean', 'bce_sum',
              'focal_gamma')

    def __init__(self, w_bce=0.0, w_focal=0.0, w_jaccard=0.0, w_sjaccard=0.0, w_dice=0.0, smooth=100.0, eps=1e-7, norm=1.0,
                 focal_mean=0, bce_sum=0, focal_gamma=2.0):
        for k, v in zip(self.FIELDS, (w_bce, w_focal, w_jaccard, w_sjaccard, w_dice, smooth, eps, norm)):
            setattr(self, k, f32(v))
        self.focal_mean, self.bce_sum, self.focal_gamma = int(focal_mean), int(bce_sum), f32(focal_gamma)

    def tuple(self):
        return tuple(getattr(self, k) for k in self.FIELDS)


def sigmoid_x(x):
    """p = sigmoid(x) and 1 - p"""
    xd = x.double()
    u = mono(X(-xd.abs()), torch.exp, L_EXP)
    ls = sub(X(xd.clamp(max=0.0)), mono(u, torch.log1p, L_LOG1P, lo=0.0))
    p = mono(ls, torch.exp, L_EXP, hi=0.0)
    omp = X(-torch.expm1(ls.v), p.e + U * (1.0 + p.e))
    return ls, p, omp


def focal_terms(e, de, gamma):
    """f = (1 - pt)^gamma e and its derivative (de: d e / d x, or None), pt = exp(-e)"""
    pt = mono(neg(e), torch.exp, L_EXP, hi=0.0)
    om = X(-torch.expm1(-e.v), pt.e + U * (1.0 + pt.e))
    if gamma == 0:
        return e, de
    F = powq(om, gamma)
    f = mul(F, e)
    if de is None:
        return f, None
    inner = add(mul(mul(mul(c_(gamma), powq(om, gamma - 1.0)), pt), e), F)
    return f, mul(inner, de)


def pix_terms(x, t, gamma=2.0):
    """-> dict of X over the pixels: p, e, de, f, df"""
    tv = X(t.double())
    ls, p, omp = sigmoid_x(x)
    e = add(neg(mul(tv, ls)), mono(p, torch.log1p, L_LOG1P, lo=0.0))
    de = mul(omp, sub_m(div(p, add(c_(1.0), p)), tv))
    f, df = focal_terms(e, de, float(gamma))
    return dict(p=p, e=e, de=de, f=f, df=df, t=tv, omp=omp)


def correct_at_half(x, t):
    """sigmoid(x) > 0.5 is x > 0 (x == 0: the tie goes to "not above")"""
    return ((x > 0) == (t != 0)).double().sum()


def binary_sums(x, t, gamma=2.0, q=None):
    """-> list of 7 X: the sums[0..6] of segnb_seg_loss_reduce (4, 5, 6 exact)"""
    q = q or pix_terms(x, t, gamma)
    return [dsum(q['e']), dsum(q['f']), dsum(mul(q['p'], q['t'])), dsum(q['p']), X(t.double().sum()),
            X(correct_at_half(x, t)), c_(x.numel())]


def add_sums(a, b):
    return [X(u.v + v.v, u.e + v.e) for u, v in zip(a, b)]


def binary_fin(S, sp):
    """-> X[8]: the result vector of segnb_seg_loss_finalize from sums with bounds"""
    n, I = S[6], S[2]
    Uu = add(S[3], S[4])
    bce = S[0] if sp.bce_sum else div(S[0], n)
    focal = div(S[1], n) if sp.focal_mean else S[1]
    eps, sm = c_(sp.eps), c_(sp.smooth)
    UI = sub(Uu, I)
    Dj, Ds, Dd = add(UI, eps), add(UI, sm), add(Uu, eps)
    jac = sub_m(c_(1.0), div(I, Dj))
    sjac = sub_m(c_(1.0), div(add(I, sm), Ds))
    dice = sub_m(c_(1.0), div(mul(c_(2.0), I), Dd))
    tot = c_(0.0)
    for w, term in ((sp.w_bce, bce), (sp.w_focal, focal), (sp.w_jaccard, jac), (sp.w_sjaccard, sjac), (sp.w_dice, dice)):
        if w != 0:
            tot = add(tot, mul(c_(w), term))
    loss = div(tot, c_(sp.norm))
    GI, GU = c_(0.0), c_(0.0)
    if sp.w_jaccard != 0:
        GI = sub(GI, mul(c_(sp.w_jaccard), div(add(Uu, eps), mul(Dj, Dj))))
        GU = add(GU, mul(c_(sp.w_jaccard), div(I, mul(Dj, Dj))))
    if sp.w_sjaccard != 0:
        GI = sub(GI, mul(c_(sp.w_sjaccard), div(add(Uu, mul(c_(2.0), sm)), mul(Ds, Ds))))
        GU = add(GU, mul(c_(sp.w_sjaccard), div(add(I, sm), mul(Ds, Ds))))
    if sp.w_dice != 0:
        GI = sub(GI, mul(c_(sp.w_dice), div(c_(2.0), Dd)))
        GU = add(GU, mul(c_(sp.w_dice), div(mul(c_(2.0), I), mul(Dd, Dd))))
    iou = div(I, add(UI, c_(1e-7)))
    acc = div(S[5], n)
    return eo.stack([_stored(v) for v in (loss, iou, acc, GI, GU, bce, n, c_(0.0))])


def _stored(x):
    """one more rounding: the float64 result stored as fp32"""
    return X(x.v, x.e + U * x.v.abs() + TINY) if float(x.e) != 0 or float(x.v) != f32(float(x.v)) else x


def binary_bwd(x, t, fin32, sp, grad_out=None, q=None):
    """dlogits of segnb_seg_loss_bwd; fin32: the fp32 result vector the call is given (exact input)"""
    q = q or pix_terms(x, t, sp.focal_gamma)
    fin = [float(v) for v in torch.as_tensor(fin32).double().reshape(-1)]
    go = div(c_(1.0 if grad_out is None else f32(grad_out)), c_(sp.norm))
    inv_n = div(c_(1.0), c_(fin[6]))
    wb = c_(sp.w_bce) if sp.bce_sum else mul(c_(sp.w_bce), inv_n)
    wf = mul(c_(sp.w_focal), inv_n) if sp.focal_mean else c_(sp.w_focal)
    dp = mul(q['p'], q['omp'])
    region = mul(dp, add(mul(q['t'], c_(fin[3])), c_(fin[4])))
    return mul(go, add(add(mul(wb, q['de']), mul(wf, q['df'])), region))


def binary_map(x, t, kind, gamma, q=None):
    q = q or pix_terms(x, t, gamma)
    return q['e'] if kind == 0 else q['f']


def binary_map_bwd(x, t, kind, gamma, gout, q=None):
    q = q or pix_terms(x, t, gamma)
    return mul(X(gout.double()), q['de'] if kind == 0 else q['df'])


def nonvacuous(x, what):
    """bound <= 1e-3 |value| on every non-zero element"""
    nz = x.v != 0
    assert bool((out_bound(x)[nz] <= 1e-3 * x.v.abs()[nz]).all()), '%s: a vacuous bound: value %s bound %s' % (
        what, x.v.tolist(), out_bound(x).tolist())


# ------------------------------------------------------------------------------------------------------------------ histogram
def hist_oracle(x, t, thr):
    """-> hist int64 [2][nthr + 1], slack int64 [2][nthr + 1] (ambiguous pixels that may enter or leave each bucket), number of
    ambiguous pixels.  x == 0 is sigmoid exactly 0.5: an exact value is never ambiguous."""
    _, p, _ = sigmoid_x(x)
    pe = torch.where(x == 0, torch.zeros_like(p.e), p.e)
    th = thr.double()
    nthr = th.numel()
    b = torch.searchsorted(th, p.v.contiguous(), right=False)                 # thresholds strictly below p
    # (0 <= sigmoid <= 1 in any implementation)
    blo = torch.searchsorted(th, (p.v - pe).clamp(min=0.0).contiguous(), right=False)
    bhi = torch.searchsorted(th, (p.v + pe).clamp(max=1.0).contiguous(), right=False)
    cls = (t != 0).long()
    hist = torch.zeros(2, nthr + 1, dtype=torch.int64)
    slack = torch.zeros(2, nthr + 2, dtype=torch.int64)
    amb = blo != bhi
    for c in (0, 1):
        hist[c] = torch.bincount(b[cls == c], minlength=nthr + 1)
        m = amb & (cls == c)
        slack[c] += torch.bincount(blo[m], minlength=nthr + 2)
        slack[c] -= torch.bincount(bhi[m] + 1, minlength=nthr + 2)
    return hist, slack.cumsum(1)[:, :nthr + 1], int(amb.sum())


def check_hist(got, hist, slack):
    got = torch.as_tensor(got).cpu().reshape(hist.shape)
    assert int(got.sum()) == int(hist.sum()), 'sum(hist) %d, pixels %d' % (int(got.sum()), int(hist.sum()))
    assert torch.equal(got.sum(1), hist.sum(1)), 'per-class totals %s vs %s' % (got.sum(1).tolist(), hist.sum(1).tolist())
    bad = (got - hist).abs() > slack
    assert not bool(bad.any()), 'buckets %s: got %s, oracle %s, ambiguous %s' % (
        bad.nonzero()[:4].tolist(), got[bad][:4].tolist(), hist[bad][:4].tolist(), slack[bad][:4].tolist())


# ------------------------------------------------------------------------------------------------------------------ absmax
def absmax_oracle(x):
    """max |x| as an fp32 number; NaN when any element is NaN"""
    if bool(torch.isnan(x).any()):
        return float('nan')
    return float(x.abs().max())


def same_float(got, want):
    got = float(got)
    return (got != got) if want != want else (got == want and got >= 0 and not np.signbit(got))


# ------------------------------------------------------------------------------------------------------------------ multi-class
class McSpec(object):
    def __init__(self, C, mode=0, ignore_index=-100, gamma=2.0, w_focal=0.0, w_nll=0.0, w_jaccard=0.0, norm=1.0, focal_mean=1,
                 reduce=1, nll_weight=None, jac_weight=None):
        self.C, self.mode, self.ignore_index = int(C), int(mode), int(ignore_index)
        self.gamma, self.w_focal, self.w_nll, self.w_jaccard, self.norm = (f32(v) for v in (gamma, w_focal, w_nll, w_jaccard, norm))
        self.focal_mean, self.reduce = int(focal_mean), int(reduce)
        self.nll_weight = None if nll_weight is None else torch.as_tensor(nll_weight, dtype=torch.float32)
        self.jac_weight = None if jac_weight is None else torch.as_tensor(jac_weight, dtype=torch.float32)

    def cfg(self):
        return (self.mode, self.ignore_index, self.gamma, self.w_focal, self.w_nll, self.w_jaccard, self.norm, self.focal_mean,
                self.reduce)


SMOOTH = 100.0


def mc_parts(x, t, sp):
    """x [N,C,HW] fp32, t [N,HW] int64 -> logp, p (X [N,C,HW]), valid, inr (bool [N,HW]), tc (labels clamped to an index where
    they are not one: never used unmasked), logpt X [N,HW]"""
    xd = x.double()
    C = x.shape[1]
    if sp.mode == 0:
        m = xd.max(1, keepdim=True).values
        ex = mono(sub(X(xd), X(m)), torch.exp, L_EXP, hi=0.0)
        s = eo.fsum(ex, 1)
        s = X(s.v, s.e + (C - 1) * (L_EXP + 2) * U * s.v)
        ls = mono(s, torch.log, L_LOG, lo=1.0)
        logp = sub_m(sub(X(xd), X(m)), X(ls.v[:, None].expand_as(xd), ls.e[:, None].expand_as(xd)))
        logp = X(torch.log_softmax(xd, 1), logp.e)
    else:
        logp = X(xd)
    p = mono(logp, torch.exp, L_EXP)
    valid = t != sp.ignore_index
    inr = valid & (t >= 0) & (t < C)
    tc = torch.where(inr, t, torch.zeros_like(t))
    logpt = X(torch.gather(logp.v, 1, tc[:, None])[:, 0], torch.gather(logp.e, 1, tc[:, None])[:, 0])
    return logp, p, valid, inr, tc, logpt


def _masked(x, m):
    z = torch.zeros((), dtype=F64)
    return X(torch.where(m, x.v, z), torch.where(m, x.e, z))


def mc_sums(x, t, sp, parts=None):
    """-> X [3C + 8]"""
    C = x.shape[1]
    logp, p, valid, inr, tc, logpt = parts or mc_parts(x, t, sp)
    onehot = torch.nn.functional.one_hot(tc, C).permute(0, 2, 1).bool() & inr[:, None]
    Ic = dsum(_masked(p, onehot).map(lambda a: a.permute(1, 0, 2).reshape(C, -1)), 1)
    Pc = dsum(_masked(p, valid[:, None].expand_as(onehot)).map(lambda a: a.permute(1, 0, 2).reshape(C, -1)), 1)
    Tc = X(onehot.double().sum((0, 2)))
    nlp = neg(logpt)
    focal, _ = focal_terms(nlp, None, sp.gamma)
    w = sp.nll_weight.double()[tc] if sp.nll_weight is not None else torch.ones_like(logpt.v)
    nll = mul(X(w), nlp)
    tail = [dsum(_masked(focal, inr)), dsum(_masked(nll, inr)), dsum(X(w * inr.double())), X(valid.double().sum()),
            c_(t.numel()), X((valid & ~inr).double().sum()), c_(0.0), c_(0.0)]
    return X(torch.cat([Ic.v, Pc.v, Tc.v, torch.stack([a.v for a in tail])]),
             torch.cat([Ic.e, Pc.e, Tc.e, torch.stack([a.e for a in tail])]))


def mc_fin(S, sp):
    """-> X [8 + 3C] from the sums with bounds"""
    C = sp.C
    I, P, T = S[0:C], S[C:2 * C], S[2 * C:3 * C]
    w = X(sp.jac_weight.double()) if sp.jac_weight is not None else X(torch.ones(C, dtype=F64))
    present = T.v > 0
    sm = c_(SMOOTH)
    D = add(sub(add(P, T), I), sm)
    D2 = mul(D, D)
    L = _masked(sub_m(c_(1.0), div(add(I, sm), D)), present)
    gI = _masked(neg(div(add(add(P, T), c_(2 * SMOOTH)), D2)), present)
    gP = _masked(div(add(I, sm), D2), present)
    jscale = div(c_(sp.w_jaccard), c_(sp.norm)) if sp.reduce else c_(1.0)
    wL = mul(w, L)
    nall, W = S[3 * C + 4], S[3 * C + 2]
    focal = div(S[3 * C], nall) if sp.focal_mean else S[3 * C]
    nll = div(S[3 * C + 1], W) if float(W.v) != 0 else X(torch.tensor(float('nan'), dtype=F64))
    loss = mul(c_(sp.w_jaccard), dsum(wL))
    if sp.w_focal != 0:
        loss = add(loss, mul(c_(sp.w_focal), focal))
    if sp.w_nll != 0:
        loss = add(loss, mul(c_(sp.w_nll), nll))
    loss = div(loss, c_(sp.norm))
    cf = div(div(c_(sp.w_focal), c_(sp.norm)), nall if sp.focal_mean else c_(1.0))
    if sp.w_nll != 0:
        cn = div(div(c_(sp.w_nll), c_(sp.norm)), W) if float(W.v) != 0 else X(torch.tensor(float('inf'), dtype=F64))
    else:
        cn = c_(0.0)
    head = [loss, cf, cn, S[3 * C + 3], nall, S[3 * C + 5], focal, nll]
    parts = [eo.stack([h for h in head]), wL, mul(mul(jscale, w), gI), mul(mul(jscale, w), gP)]
    v, e = torch.cat([a.v for a in parts]), torch.cat([a.e for a in parts])
    return X(v, torch.where((e != 0) | (v.float().double() != v), e + U * v.abs() + TINY, e))


def mc_bwd(x, t, sp, fin32, gout=None, parts=None):
    """dlogits of segnb_mc_loss_bwd -> X [N,C,HW]; fin32 the fp32 vector the call is given, gout fp32 [1] or [C] or None"""
    C = x.shape[1]
    logp, p, valid, inr, tc, logpt = parts or mc_parts(x, t, sp)
    fin = torch.as_tensor(fin32).double().reshape(-1)
    g = torch.ones(1, dtype=F64) if gout is None else torch.as_tensor(gout).double().reshape(-1)
    gc = X(g if not sp.reduce else g[:1].expand(C))
    cI = mul(gc, X(fin[8 + C:8 + 2 * C]))
    cP = mul(gc, X(fin[8 + 2 * C:8 + 3 * C]))
    cf, cn = mul(c_(g[0]), c_(fin[1])), mul(c_(g[0]), c_(fin[2]))
    nlp = neg(logpt)
    # d focal / d logpt = -d/d(e) [(1 - pt)^gamma e] at e = -logpt
    _, dfoc = focal_terms(nlp, c_(-1.0), sp.gamma)
    a = mul(cf, dfoc)
    if sp.w_nll != 0 and float(cn.v) != 0:
        w = sp.nll_weight.double()[tc] if sp.nll_weight is not None else torch.ones_like(logpt.v)
        a = sub(a, mul(cn, X(w)))
    a = _masked(a, inr)
    a = X(a.v[:, None], a.e[:, None])
    onehot = torch.nn.functional.one_hot(tc, C).permute(0, 2, 1).bool() & inr[:, None]
    cIb = X(cI.v[None, :, None], cI.e[None, :, None])
    cPb = X(cP.v[None, :, None], cP.e[None, :, None])
    gj = _masked(add(cPb, _masked(X(cIb.v.expand(onehot.shape), cIb.e.expand(onehot.shape)), onehot)),
                 valid[:, None].expand_as(onehot))
    oh = X(onehot.double())
    if sp.mode == 0:
        S = eo.fsum(mul(p, gj), 1)
        S = X(S.v[:, None], S.e[:, None])
        return add(sub_m(mul(a, oh), mul(a, p)), mul(p, sub_m(gj, S)))
    return add(mul(a, oh), mul(p, gj))


# ------------------------------------------------------------------------------------------------------------------ records
class Recorder(object):
    """worst err / bound per (entry point, case family) of the cases run in this process: the figures kept in PROFILE"""
    def __init__(self):
        self.rows = {}

    def add(self, key, worst, extra=''):
        w, _ = self.rows.get(key, (0.0, ''))
        self.rows[key] = (max(w, worst), extra)

    def lines(self):
        return ['%-44s worst err/bound %.4f %s' % (k, w, x) for k, (w, x) in sorted(self.rows.items())]


# ------------------------------------------------------------------------------------------------------------------ cases
# The shared runner: `dev` is 'cuda' (the library) or 'cpu' (a backend installed with segnb._native.set_backend_for_testing);
# every call goes through segnb._native.call on raw pointers, as tests/test_gcn_gpu.py calls its ABI.
PLANT = [0.0, 1e-3, -1e-3, 8.3, -8.3, 16.7, -16.7, 17.4, -17.4, 40.0, -40.0, 88.7, -88.7, 89.0, -89.0, 104.0, -104.0, 1e4, -1e4]
BINARY_N = [1, 3, 4, 5, 255, 1023, 1024, 1025, 8 * 1024 + 5, 524288, 524288 + 1029, 1572864 + 3]
SMALL_N = [n for n in BINARY_N if n <= 8 * 1024 + 5]
LARGE_N = [n for n in BINARY_N if n > 8 * 1024 + 5]
GAMMAS = [2.0, 0.0, 1.0, 1.5, 3.0, 0.5]
NAMED_SPECS = {
    'dice': dict(w_dice=1.0), 'jaccard': dict(w_jaccard=1.0), 'smooth_jaccard': dict(w_sjaccard=1.0, smooth=100.0),
    'bce': dict(w_bce=1.0), 'bce_smooth_jaccard': dict(w_bce=1.0, w_sjaccard=0.5, smooth=100.0),
    'bce_dice': dict(w_bce=0.7, w_dice=0.3, norm=1.0), 'focal': dict(w_focal=1.0, focal_mean=1),
    'bce_sum': dict(w_bce=1.0, bce_sum=1), 'focal_sum_g15': dict(w_focal=1.0, focal_mean=0, focal_gamma=1.5),
    'focal_g05': dict(w_focal=1.0, focal_mean=1, focal_gamma=0.5), 'focal_g0': dict(w_focal=1.0, focal_mean=1, focal_gamma=0.0),
    'all_norm3': dict(w_bce=0.5, w_focal=0.25, w_jaccard=1.0, w_sjaccard=0.5, w_dice=0.75, norm=3.0, focal_mean=1,
                      focal_gamma=3.0),
}


def binary_data(n, seed=0, labels='01'):
    """3 * randn with the planted logits at the head (under both labels), in the last elements and behind element 524288 (the
    second grid-stride trip of a 512-block launch); x == 0 planted, no other |x| below 1e-6"""
    g = torch.Generator().manual_seed(1000 * seed + n % 997)
    x = 3.0 * torch.randn(n, generator=g)
    x[x.abs() < 1e-6] = 1e-3
    t = torch.randint(0, 2, (n,), generator=g)
    pv = torch.tensor(PLANT, dtype=torch.float32)
    k = len(PLANT)
    if n < 2 * k:
        idx = torch.arange(n)
        x.copy_(pv[(idx + seed) % k])
        t.copy_((idx + seed) // k % 2 if n > 1 else torch.tensor([seed % 2]))
    else:
        x[:k], t[:k] = pv, 0
        x[k:2 * k], t[k:2 * k] = pv, 1
        x[n - k:] = pv.flip(0)
        t[n - k:] = torch.arange(k) % 2
        if n >= 524288 + 2 * k:
            x[524288:524288 + k] = pv
            t[524288:524288 + k] = (torch.arange(k) + 1) % 2
    if labels == 'mixed':
        r = torch.rand(n, generator=g)
        t[r < 0.02] = 2
        t[r > 0.98] = 255
        if n >= 2 * k:
            t[1:k:3] = 255
            t[k + 1:2 * k:3] = 2
            t[n - 2] = 255
    return x, t


def placed(t, dev, off=0):
    """the tensor on `dev` behind `off` leading elements of its own type (off = 1: a float one float, an int64 8 bytes, off the
    16-byte alignment of the allocation)"""
    buf = torch.zeros(t.numel() + off, dtype=t.dtype, device=dev)
    buf[off:] = t.to(dev)
    return buf[off:]


def _nv():
    from segnb import _native as nv
    return nv


def _stream(dev):
    return torch.cuda.current_stream().cuda_stream if dev == 'cuda' else 0


def _sync(dev):
    if dev == 'cuda':
        torch.cuda.synchronize()


def cspec(sp):
    nv = _nv()
    s = nv.LossSpec()
    for k, v in zip(Spec.FIELDS, sp.tuple()):
        setattr(s, k, v)
    return s


def call_map(dev, x, t, kind, gamma):
    nv = _nv()
    out = torch.full((x.numel() + 1,), 7.0, dtype=torch.float32, device=dev)
    nv.call('segnb_seg_loss_map', nv.ptr(x), nv.ptr(t), x.numel(), kind, float(gamma), nv.ptr(out), _stream(dev))
    _sync(dev)
    assert float(out[-1]) == 7.0, 'a write past the end'
    return out[:-1].cpu()


def call_map_bwd(dev, x, t, kind, gamma, gout):
    nv = _nv()
    out = torch.full((x.numel() + 1,), 7.0, dtype=torch.float32, device=dev)
    g = gout.to(dev)
    nv.call('segnb_seg_loss_map_bwd', nv.ptr(x), nv.ptr(t), x.numel(), kind, float(gamma), nv.ptr(g), nv.ptr(out), _stream(dev))
    _sync(dev)
    assert float(out[-1]) == 7.0, 'a write past the end'
    return out[:-1].cpu()


def call_bwd(dev, x, t, fin32, sp, grad_out, off=0):
    nv = _nv()
    n = x.numel()
    buf = torch.full((n + off + 1,), 7.0, dtype=torch.float32, device=dev)
    fin = fin32.float().to(dev)
    go = None if grad_out is None else torch.tensor([grad_out], dtype=torch.float32, device=dev)
    sums = torch.zeros(8, dtype=torch.float64, device=dev)
    nv.call('segnb_seg_loss_bwd', nv.ptr(x), nv.ptr(t), n, nv.ptr(sums), nv.ptr(fin), cspec(sp), nv.ptr(go), nv.ptr(buf, off),
            _stream(dev))
    _sync(dev)
    assert float(buf[-1]) == 7.0 and (off == 0 or float(buf[0]) == 7.0), 'a write outside dlogits'
    return buf[off:off + n].cpu()


def call_reduce(dev, x, t, gamma, sums=None):
    nv = _nv()
    if sums is None:
        sums = torch.zeros(8, dtype=torch.float64, device=dev)
    nv.call('segnb_seg_loss_reduce', nv.ptr(x), nv.ptr(t), x.numel(), float(gamma), nv.ptr(sums), _stream(dev))
    _sync(dev)
    return sums


def call_finalize(dev, sums, sp):
    nv = _nv()
    fin = torch.zeros(8, dtype=torch.float32, device=dev)
    nv.call('segnb_seg_loss_finalize', nv.ptr(sums), cspec(sp), nv.ptr(fin), _stream(dev))
    _sync(dev)
    return fin.cpu()


def call_one_launch(dev, x, t, sp, work):
    nv = _nv()
    fin = torch.zeros(8, dtype=torch.float32, device=dev)
    nv.call('segnb_seg_loss_reduce_finalize', nv.ptr(x), nv.ptr(t), x.numel(), cspec(sp), nv.ptr(work), nv.ptr(fin), _stream(dev))
    _sync(dev)
    return fin.cpu()


def check_sums(got, S, what):
    """the 7 sums against the oracle: integers with ==, the rest within the bound -> worst err / bound"""
    got = got.detach().cpu().double()
    for k in (4, 5, 6):
        assert float(got[k]) == float(S[k].v), '%s: sums[%d] = %r, oracle %r' % (what, k, float(got[k]), float(S[k].v))
    assert float(got[7]) == 0.0
    worst = 0.0
    for k in (0, 1, 2, 3):
        r = ratio(got[k], S[k])
        assert r <= 1.0, '%s: sums[%d] = %r, oracle %r, err/bound %.3g' % (what, k, float(got[k]), float(S[k].v), r)
        worst = max(worst, r)
    return worst


def check_fin(got, F, what):
    got = got.detach().cpu().double()
    assert float(got[6]) == float(F.v[6]) and float(got[7]) == 0.0, what
    assert float(got[2]) == f32(float(F.v[2])), '%s: accuracy %r vs %r' % (what, float(got[2]), float(F.v[2]))
    r = ratio(got[:6], F[:6])
    assert r <= 1.0, '%s: fin %s, oracle %s, bound %s' % (what, got[:6].tolist(), F.v[:6].tolist(), out_bound(F)[:6].tolist())
    return r


def fin_nonvacuous(F, what):
    """the loss and every non-zero gradient coefficient"""
    nonvacuous(X(F.v[[0, 3, 4]], F.e[[0, 3, 4]]), what)


# ------------------------------------------------------------------------------------------------------------------ multi-class
def mc_data(N, C, HW, seed, kind='randn', mode=0, ignore_index=-1, bad=True, absent=True, lead=None, offset=0.0):
    """x [N,C,HW] fp32, t [N,HW] int64.  mode 1: log-probabilities (log_softmax of the draw, rounded to fp32), with pixels whose
    target log-probability is exactly 0 and others at -1e4.  lead: the target's logit leads the rest of some pixels by 16.7,
    17.4 and 200.  10 % of the pixels carry ignore_index, a few carry labels on either side of [0, C)."""
    g = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(N, C, HW, generator=g)
    t = torch.randint(0, C, (N, HW), generator=g)
    if absent and C > 2:
        t[t == 2] = 0                                       # class 2 absent from the targets
    npx = N * HW
    tf, lin = t.view(-1), torch.arange(npx)
    n_i, hw_i = lin // HW, lin % HW
    if lead or mode == 1:
        leads = torch.tensor([16.7, 17.4, 200.0])
        sel = lin % 5 == 1
        cls = tf[sel]
        xs = x[n_i[sel], :, hw_i[sel]]
        top = xs.max(1).values + leads[torch.arange(int(sel.sum())) % 3]
        xs[torch.arange(xs.shape[0]), cls] = top
        x[n_i[sel], :, hw_i[sel]] = xs
    if offset:
        x = x + offset
    if mode == 1:
        x = torch.log_softmax(x.double(), 1).float()
        z = lin % 10 == 3                                   # log-probabilities of exactly 0 (target) and -1e4 (the rest)
        xs = torch.full((int(z.sum()), C), -1e4)
        xs[torch.arange(xs.shape[0]), tf[z]] = 0.0
        x[n_i[z], :, hw_i[z]] = xs
        if C > 1:
            w = lin % 10 == 7                               # the target itself at -1e4
            xs = x[n_i[w], :, hw_i[w]]
            xs[torch.arange(xs.shape[0]), tf[w]] = -1e4
            x[n_i[w], :, hw_i[w]] = xs
    t[torch.rand(N, HW, generator=g) < 0.1] = ignore_index
    if bad and npx >= 8:
        tf[0] = C + 3
        tf[npx - 1] = -7 if ignore_index != -7 else -8
        tf[npx // 2] = C
    return x.contiguous(), t.contiguous()


def mc_cspec(sp, dev, keep):
    nv = _nv()
    s = nv.McLossSpec()
    s.C, s.mode, s.ignore_index, s.gamma = sp.C, sp.mode, sp.ignore_index, sp.gamma
    s.w_focal, s.w_nll, s.w_jaccard, s.norm = sp.w_focal, sp.w_nll, sp.w_jaccard, sp.norm
    s.focal_mean, s.reduce = sp.focal_mean, sp.reduce
    for k in ('nll_weight', 'jac_weight'):
        w = getattr(sp, k)
        if w is not None:
            w = w.to(dev)
            keep.append(w)
        setattr(s, k, nv.ptr(w))
    return s


def mc_work(dev, C):
    nv = _nv()
    return torch.zeros(int(nv.query('segnb_mc_loss_work_doubles', C)), dtype=torch.float64, device=dev)


def mc_call_forward(dev, x, t, sp, work, one_launch):
    """-> (sums or None, fin) on the CPU"""
    nv = _nv()
    N, C, HW = x.shape
    keep = []
    cs = mc_cspec(sp, dev, keep)
    fin = torch.zeros(8 + 3 * C, dtype=torch.float32, device=dev)
    st = _stream(dev)
    if one_launch:
        nv.call('segnb_mc_loss_reduce_finalize', nv.ptr(x), nv.ptr(t), N, HW, cs, nv.ptr(work), nv.ptr(fin), st)
        _sync(dev)
        return None, fin.cpu()
    sums = torch.full((3 * C + 8,), 5.0, dtype=torch.float64, device=dev)
    nv.call('segnb_mc_loss_reduce', nv.ptr(x), nv.ptr(t), N, HW, cs, nv.ptr(work), nv.ptr(sums), st)
    nv.call('segnb_mc_loss_finalize', nv.ptr(sums), cs, nv.ptr(fin), st)
    _sync(dev)
    return sums.cpu(), fin.cpu()


def mc_call_bwd(dev, x, t, sp, fin32, gout):
    nv = _nv()
    N, C, HW = x.shape
    keep = []
    cs = mc_cspec(sp, dev, keep)
    fin = fin32.float().to(dev)
    g = None if gout is None else gout.float().to(dev)
    dx = torch.full((N * C * HW + 1,), 7.0, dtype=torch.float32, device=dev)
    nv.call('segnb_mc_loss_bwd', nv.ptr(x), nv.ptr(t), N, HW, cs, nv.ptr(fin), nv.ptr(g), nv.ptr(dx), _stream(dev))
    _sync(dev)
    assert float(dx[-1]) == 7.0, 'a write past the end'
    return dx[:-1].view(N, C, HW).cpu()


def mc_check_sums(got, S, C, what):
    got = got.detach().cpu().double()
    exact = list(range(2 * C, 3 * C)) + [3 * C + 3, 3 * C + 4, 3 * C + 5, 3 * C + 6, 3 * C + 7]
    assert torch.equal(got[exact], S.v[exact]), '%s: integer sums %s vs %s' % (what, got[exact].tolist(), S.v[exact].tolist())
    real = [i for i in range(3 * C + 8) if i not in exact]
    r = ratio(got[real], X(S.v[real], S.e[real]))
    assert r <= 1.0, '%s: real sums err/bound %.3g' % (what, r)
    return r


def mc_check_fin(got, F, C, what, nll_defined=True):
    got = got.detach().cpu().double()
    assert torch.equal(got[3:6], F.v[3:6]), '%s: counts %s vs %s' % (what, got[3:6].tolist(), F.v[3:6].tolist())
    idx = [i for i in range(8 + 3 * C) if i not in (3, 4, 5) and (nll_defined or i not in (0, 2, 7))]
    r = ratio(got[idx], X(F.v[idx], F.e[idx]))
    assert r <= 1.0, '%s: fin err/bound %.3g: got %s oracle %s' % (what, r, got[idx][:12].tolist(), F.v[idx][:12].tolist())
    return r


def mc_fin_nonvacuous(F, sp, what):
    C = sp.C
    idx = [0, 1, 2] + list(range(8 + C, 8 + 3 * C))
    nonvacuous(X(F.v[idx], F.e[idx]), what)


# ------------------------------------------------------------------------------------------------------------------ test bodies
# shared by tests/test_loss_oracle_gpu.py (dev = 'cuda') and tests/test_loss_oracle_cpu.py (dev = 'cpu', an fp32 backend)
REC = Recorder()
ALIGNS = ('aligned', 'logits+1', 'target+1', 'dlogits+1')


def _bwd_spec(gamma, i):
    return Spec(w_bce=0.5, w_focal=0.25, w_jaccard=1.0, w_sjaccard=0.5, w_dice=0.75, norm=(3.0, 1.0)[i % 2], focal_mean=i % 2,
                bce_sum=(i // 2) % 2, focal_gamma=gamma)


def case_binary_pixels(dev, n, align, gammas, labels='mixed'):
    """map, map_bwd and bwd: every element within its bound, nothing non-finite"""
    x, t = binary_data(n, ALIGNS.index(align), labels)
    xd = placed(x, dev, 1 if align == 'logits+1' else 0)
    td = placed(t, dev, 1 if align == 'target+1' else 0)
    gout = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 2
    fam = 'n<=8197' if n <= 8197 else 'n>=524288'
    for i, gamma in enumerate(gammas):
        q = pix_terms(x, t, gamma)
        for kind in (0, 1):
            r = ratio(call_map(dev, xd, td, kind, gamma), binary_map(x, t, kind, gamma, q))
            assert r <= 1.0, 'map kind %d gamma %g n %d %s: err/bound %.3g' % (kind, gamma, n, align, r)
            REC.add('seg_loss_map kind%d %s' % (kind, fam), r)
            r = ratio(call_map_bwd(dev, xd, td, kind, gamma, gout), binary_map_bwd(x, t, kind, gamma, gout, q))
            assert r <= 1.0, 'map_bwd kind %d gamma %g n %d %s: err/bound %.3g' % (kind, gamma, n, align, r)
            REC.add('seg_loss_map_bwd kind%d %s' % (kind, fam), r)
        sp = _bwd_spec(gamma, i)
        fin32 = binary_fin(binary_sums(x, t, gamma, q), sp).v.float()
        go = None if i % 2 == 0 else 1.7
        got = call_bwd(dev, xd, td, fin32, sp, go, 1 if align == 'dlogits+1' else 0)
        r = ratio(got, binary_bwd(x, t, fin32, sp, go, q))
        assert r <= 1.0, 'bwd gamma %g n %d %s: err/bound %.3g' % (gamma, n, align, r)
        REC.add('seg_loss_bwd %s' % fam, r)


def case_binary_reduce(dev, n, specname, align='aligned', labels=None):
    """two-launch and one-launch forms against the oracle and against each other; the work buffer left zero.  Labels 0/1 with a
    sprinkling of 2 and 255 under the specs that weigh every term; the single-term specs keep 0/1 (a region loss of its own is
    1 - 2 I / U, which labels of 255 bring next to 0: no relative bound could be asked of it)"""
    sp = Spec(**NAMED_SPECS[specname])
    labels = labels or ('mixed' if specname in ('all_norm3', 'focal_g05', 'bce_sum') else '01')
    x, t = binary_data(n, 3 + ALIGNS.index(align), labels)
    xd = placed(x, dev, 1 if align == 'logits+1' else 0)
    td = placed(t, dev, 1 if align == 'target+1' else 0)
    S = binary_sums(x, t, sp.focal_gamma)
    F = binary_fin(S, sp)
    what = '%s n=%d %s' % (specname, n, align)
    fam = 'n<=8197' if n <= 8197 else 'n>=524288'
    fin_nonvacuous(F, what)
    sums = call_reduce(dev, xd, td, sp.focal_gamma)
    REC.add('seg_loss_reduce %s' % fam, check_sums(sums, S, what))
    fin2 = call_finalize(dev, sums, sp)
    REC.add('seg_loss_finalize %s' % fam, check_fin(fin2, F, what + ' two-launch'))
    work = torch.zeros(128, dtype=torch.float64, device=dev)
    fin1 = call_one_launch(dev, xd, td, sp, work)
    REC.add('seg_loss_reduce_finalize %s' % fam, check_fin(fin1, F, what + ' one-launch'))
    assert not bool(work.cpu().view(torch.int64).any()), what + ': the work buffer is not all zero after the call'
    assert bool(((fin1.double() - fin2.double()).abs()[:6] <= 2 * out_bound(F)[:6]).all()), (what, fin1.tolist(), fin2.tolist())


def case_binary_work_reuse(dev, ns=(1025, 8 * 1024 + 5, 524288 + 1029)):
    """consecutive calls of different n on one work buffer: each matches its own oracle"""
    sp = Spec(**NAMED_SPECS['all_norm3'])
    work = torch.zeros(128, dtype=torch.float64, device=dev)
    for n in ns:
        x, t = binary_data(n, 5, '01')
        F = binary_fin(binary_sums(x, t, sp.focal_gamma), sp)
        fin = call_one_launch(dev, placed(x, dev), placed(t, dev), sp, work)
        REC.add('seg_loss_reduce_finalize reuse', check_fin(fin, F, 'work reuse n=%d' % n))
        assert not bool(work.cpu().view(torch.int64).any()), 'n=%d: the work buffer is not all zero after the call' % n


def case_binary_halves(dev, n):
    """the data-parallel contract: two calls on the halves into one `sums` equal one call on the whole"""
    x, t = binary_data(n, 6, 'mixed')
    xd, td = placed(x, dev), placed(t, dev)
    h = n // 2 + 1
    S = binary_sums(x, t, 2.0)
    whole = call_reduce(dev, xd, td, 2.0)
    halves = call_reduce(dev, xd[:h], td[:h], 2.0)
    halves = call_reduce(dev, xd[h:], td[h:], 2.0, halves)
    REC.add('seg_loss_reduce halves', max(check_sums(whole, S, 'whole n=%d' % n), check_sums(halves, S, 'halves n=%d' % n)))
    assert torch.equal(whole.cpu()[4:], halves.cpu()[4:])


def case_binary_degenerate(dev, n=1025):
    """closed forms where a relative bound cannot be asked for"""
    eps = f32(1e-7)
    # empty target, logits at -90: I = 0 exactly, sum p < n * 2^-126: Jaccard D = eps, loss 1, GI = -1 / eps, GU = 0
    x, t = torch.full((n,), -90.0), torch.zeros(n, dtype=torch.int64)
    work = torch.zeros(128, dtype=torch.float64, device=dev)
    fin = call_one_launch(dev, placed(x, dev), placed(t, dev), Spec(w_jaccard=1.0), work).double()
    assert float(fin[0]) == 1.0 and float(fin[1]) == 0.0 and float(fin[2]) == 1.0 and float(fin[4]) == 0.0, fin.tolist()
    assert abs(float(fin[3]) + 1.0 / eps) <= 2 * U / eps, fin.tolist()
    # all-ones target, logits at +90: p == 1, I = n, U = 2n: jaccard = eps / (n + eps), dice = eps / (2n + eps); in float64
    # 1 - n / (n + eps) carries 2^-53 absolute, 2^-53 n / eps relative (1.1e-6 at n = 1025): 1e-5 asked
    x, t = torch.full((n,), 90.0), torch.ones(n, dtype=torch.int64)
    fin = call_one_launch(dev, placed(x, dev), placed(t, dev), Spec(w_jaccard=1.0), work).double()
    want = eps / (n + eps)
    assert abs(float(fin[0]) - want) <= 1e-5 * want and float(fin[1]) == 1.0 and float(fin[2]) == 1.0, (fin.tolist(), want)
    fin = call_one_launch(dev, placed(x, dev), placed(t, dev), Spec(w_dice=1.0), work).double()
    want = eps / (2 * n + eps)
    assert abs(float(fin[0]) - want) <= 1e-5 * want, (fin.tolist(), want)
    assert abs(float(fin[3]) + 2.0 / (2 * n + eps)) <= 4 * U / n and abs(float(fin[4]) - 2.0 * n / (2 * n + eps) ** 2) <= 4 * U / n


def _bits(t):
    return t.contiguous().view(torch.int32)


def case_mc(dev, C, N, HW, mode=0, gamma=2.0, ignore_index=-1, off=0, data=None, degenerate=False, **spec):
    """reduce + finalize (two launches, one launch, repeated: bitwise equal) and bwd against the oracle"""
    data = dict(data or {})
    sp = McSpec(C, mode=mode, ignore_index=ignore_index, gamma=gamma, **spec)
    x, t = mc_data(N, C, HW, seed=C * 131 + HW, mode=mode, ignore_index=ignore_index, **data)
    xd = placed(x.view(-1), dev, off).view(N, C, HW)
    td = t.to(dev)
    what = 'C=%d N=%d HW=%d mode=%d gamma=%g ign=%d off=%d %s %s' % (C, N, HW, mode, gamma, ignore_index, off, data, sorted(spec))
    fam = 'mode%d' % mode
    parts = mc_parts(x, t, sp)
    S = mc_sums(x, t, sp, parts)
    F = mc_fin(S, sp)
    if not degenerate:
        mc_fin_nonvacuous(F, sp, what)
    work = mc_work(dev, C)
    sums, fin2 = mc_call_forward(dev, xd, td, sp, work, False)
    REC.add('mc_loss_reduce %s' % fam, mc_check_sums(sums, S, C, what))
    REC.add('mc_loss_finalize %s' % fam, mc_check_fin(fin2, F, C, what))
    _, fin1 = mc_call_forward(dev, xd, td, sp, work, True)
    _, fin1b = mc_call_forward(dev, xd, td, sp, work, True)
    assert torch.equal(_bits(fin1), _bits(fin2)), what + ': one launch and two launches differ'
    assert torch.equal(_bits(fin1), _bits(fin1b)), what + ': a repeated call differs'
    if C == 1 and mode == 0:
        # one class: p == 1 at every pixel, I = T = the in-range pixels, P = the valid ones, all exact: the closed form
        nin, nval = float(S.v[2]), float(S.v[1])
        want = 1.0 - (nin + SMOOTH) / (nval + SMOOTH)
        assert abs(float(fin1[8]) - want) <= U * abs(want) + 2.0 ** -52, (float(fin1[8]), want)
        assert float(fin1[6]) == 0.0 and float(fin1[7]) == 0.0
    fin32 = F.v.float()
    g = torch.Generator().manual_seed(C)
    gout = torch.tensor([1.3]) if sp.reduce else torch.rand(C, generator=g) + 0.5
    dx = mc_call_bwd(dev, xd, td, sp, fin32, gout)
    r = ratio(dx, mc_bwd(x, t, sp, fin32, gout, parts))
    assert r <= 1.0, what + ': dlogits err/bound %.3g' % r
    REC.add('mc_loss_bwd %s' % fam, r)
    assert torch.equal(_bits(dx), _bits(mc_call_bwd(dev, xd, td, sp, fin32, gout))), what + ': a repeated bwd differs'
    return F, fin1, dx


def case_mc_work_reuse(dev, C=5, HW=1031, Ns=(1, 17, 4)):
    """consecutive calls of one C and different N on one work buffer"""
    sp = McSpec(C, ignore_index=-1, gamma=2.0, w_focal=1.0, w_jaccard=1.0, norm=2.0)
    work = mc_work(dev, C)
    for N in Ns:
        x, t = mc_data(N, C, HW, seed=N)
        F = mc_fin(mc_sums(x, t, sp), sp)
        _, fin = mc_call_forward(dev, placed(x.view(-1), dev).view(N, C, HW), t.to(dev), sp, work, True)
        REC.add('mc_loss_reduce_finalize reuse', mc_check_fin(fin, F, C, 'work reuse N=%d' % N))


def case_mc_all_ignored(dev, C=5, N=2, HW=37):
    """every pixel ignored: all sums but the pixel count are 0, the focal and Jaccard terms and dlogits are exactly 0; the NLL
    term is 0 / 0 = NaN (include/segnb_mc_loss.h), which is what torch.nn.NLLLoss returns"""
    x, _ = mc_data(N, C, HW, seed=1)
    t = torch.full((N, HW), 255, dtype=torch.int64)
    xd, td = placed(x.view(-1), dev).view(N, C, HW), t.to(dev)
    for w_nll in (0.0, 1.0):
        sp = McSpec(C, ignore_index=255, gamma=2.0, w_focal=1.0, w_nll=w_nll, w_jaccard=1.0)
        sums, fin = mc_call_forward(dev, xd, td, sp, mc_work(dev, C), False)
        assert float(sums[3 * C + 4]) == N * HW and not bool(sums[:3 * C + 4].any()) and not bool(sums[3 * C + 5:].any())
        assert float(fin[6]) == 0.0 and not bool(fin[8:].any()) and float(fin[3]) == 0.0 and float(fin[4]) == N * HW
        assert bool(torch.isnan(fin[7]))
        assert float(fin[0]) == 0.0 if w_nll == 0 else bool(torch.isnan(fin[0])), fin[:8].tolist()
        dx = mc_call_bwd(dev, xd, td, sp, fin, torch.tensor([1.3]))
        assert not bool(dx.view(torch.int32).bitwise_and(0x7fffffff).any()), 'dlogits of ignored pixels'


def case_hist(dev, n, nthr, seed=0, two_calls=False):
    """counts up to the ambiguous pixels of each bucket; the table holds exactly 0.5 and every 11th logit is exactly 0"""
    if nthr == 1:
        thr = torch.tensor([0.5])
    else:
        thr = torch.linspace(0, 1, nthr, dtype=torch.float64).float()       # (odd nthr: 0.5 is in the table)
        if nthr % 2 == 0:
            thr[nthr // 2] = 0.5
            thr = thr.sort().values
    assert bool((thr == 0.5).any())
    x, t = binary_data(n, 7 + seed, 'mixed')
    x[torch.arange(n) % 11 == 0] = 0.0
    hist, slack, namb = hist_oracle(x, t, thr)
    assert namb <= MAX_AMBIGUOUS * n + 1, '%d of %d pixels ambiguous' % (namb, n)
    nv = _nv()
    H = torch.zeros(2, nthr + 1, dtype=torch.int64, device=dev)
    xd, td, thd = placed(x, dev), placed(t, dev), thr.to(dev)
    if two_calls:
        h = n // 2 + 1
        nv.call('segnb_pr_histogram', nv.ptr(xd), nv.ptr(td), h, nv.ptr(thd), nthr, nv.ptr(H), _stream(dev))
        nv.call('segnb_pr_histogram', nv.ptr(xd, h), nv.ptr(td, h), n - h, nv.ptr(thd), nthr, nv.ptr(H), _stream(dev))
    else:
        nv.call('segnb_pr_histogram', nv.ptr(xd), nv.ptr(td), n, nv.ptr(thd), nthr, nv.ptr(H), _stream(dev))
    _sync(dev)
    check_hist(H, hist, slack)
    REC.add('pr_histogram n=%d nthr=%d%s' % (n, nthr, ' two calls' if two_calls else ''), 0.0,
            '(counts): %d ambiguous pixels' % namb)
    return namb


ABSMAX_N = [1, 5, 4 * 257 + 3, 1024 * 256 * 16 + 3 + 4 * 1000]


def absmax_inputs(n):
    """(name, x) pairs: the maximum in the last (tail) element and in the second grid-stride trip, -0.0, denormals, +-inf, NaN"""
    g = torch.Generator().manual_seed(n)
    base = torch.randn(n, generator=g)
    out = []
    a = base.clone(); a[n - 1] = -77.0; out.append(('max in the last element', a))
    a = base.clone(); a[n - 1 - (n > 4)] = 99.0; out.append(('max next to the end', a))
    if n > 1024 * 256 * 16:
        a = base.clone(); a[1024 * 256 * 16 + 1] = -123.0; out.append(('max in the second trip', a))
    out.append(('all -0.0', torch.full((n,), -0.0)))
    a = torch.zeros(n); a[n // 2] = -1e-41; a[0] = 3e-42; out.append(('denormals', a))
    a = base.clone(); a[n // 2] = float('-inf'); out.append(('-inf', a))
    a = base.clone(); a[0] = float('inf'); out.append(('+inf', a))
    a = base.clone(); a[n - 1] = float('nan'); out.append(('NaN in the last element', a))
    a = base.clone(); a[n // 3] = float('inf'); a[n // 2] = -float('nan'); out.append(('NaN next to inf', a))
    return out


def case_absmax(dev, n):
    nv = _nv()
    for name, x in absmax_inputs(n):
        xd = placed(x, dev)
        out = torch.full((2,), 7.0, dtype=torch.float32, device=dev)
        nv.call('segnb_absmax_f32', nv.ptr(xd), n, nv.ptr(out), _stream(dev))
        _sync(dev)
        want = absmax_oracle(x)
        assert same_float(out[0], want) and float(out[1]) == 7.0, 'absmax n=%d %s: got %r, want %r' % (n, name, float(out[0]), want)
    REC.add('absmax_f32', 0.0, '(exact)')
