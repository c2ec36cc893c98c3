"""What the element-wise entry points of libsegnb_hip.so write and refuse, as data: the cases of tests/test_ew_table_gpu.py and
the functions that run them (BatchNorm family, classifier heads, optimizer steps, add / MaxPool2d / bilinear upsampling / layout
moves, the three input / weight packers with a dtype argument).

Run as a script on the commit whose behaviour is to be pinned (the PARENT of a change to the host side of csrc/norm_act.hip,
csrc/elementwise.hip, csrc/head_loss.hip):

    python tests/ew_table.py tests/ew_table_parent.json

It runs everything twice and refuses to write a table the library does not repeat itself.

Every activation-shaped tensor is a view of Cp channels with row stride Cp + 8 into a buffer filled with a sentinel; the digest
covers the whole buffer, so a write outside the view shows.  Every input is a multiple of 1/4 (coefficients and multipliers
included, LeakyReLU slope 1/4): the per-channel sums are then exact in fp32 / fp64, and the atomically accumulated tables do not
depend on the order in which the blocks arrive.
"""
import ctypes
import hashlib
import json
import os
import sys

if __name__ == '__main__':
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(_ROOT, 'segmentation-networks-benchmark_amd'), _ROOT]

import torch

from segnb import _native as nv

JSON_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ew_table_parent.json')
DEVICE = 'cuda:0'
SLOPE, EPS, MOM, SENTINEL = 0.25, 1e-5, 0.125, 7.0
DTYPES = ('bf16', 'f32')

# BN_CASES of tests/test_hip_ops.py: N, H, W, C, act, pool, up, drop
SHAPES = [
    (2, 8, 8, 32, nv.ACT_RELU, True, False, True),        # pooled + dropout table
    (3, 7, 9, 20, nv.ACT_RELU, True, False, False),       # odd sizes, padded channels (20 -> 24), pooled
    (2, 6, 10, 96, nv.ACT_RELU, False, True, True),       # 12 chunks: not a power of two; upsampled source
    (2, 12, 12, 264, nv.ACT_LEAKY, False, False, False),  # > 32 chunks: two chunk tiles, several blocks along x
    (1, 16, 16, 8, nv.ACT_NONE, True, True, False),       # no activation, pooled + upsampled
]
HEAD_SHAPES = (0, 4)            # Cp / 8 a power of two (segnb_head_fused_ok)
# a branch that no small shape reaches, and the gate that keeps it away
UNREACHED = {'maxpool_bwd_idx_kernel<T, false>': 'maxpool_bwd_impl: N * H * W * Cp / 8 >= 2^31 items'}
# outputs that may be left out of the digests when the parent does not repeat them: per-channel tables summed with atomics
EXCLUDABLE = ('stats', 'sums', 'out_stats', 'dbias')
PIXEL_OUTPUTS = ('out', 'pool_out', 'up_out', 'dz', 'dy', 'da', 'dx', 'logits')
EXCLUDED = {}                   # {(row, output): reason}; empty: the parent repeats every table on these inputs


def pad8(c):
    return (c + 7) // 8 * 8


class V(object):
    """a [pixels][Cp] view with row stride ld = Cp + 8 of a sentinel-filled buffer"""
    def __init__(self, buf, ld):
        self.buf, self.ld, self.ptr = buf, ld, buf.data_ptr()


def P(v):
    return None if v is None else (v.ptr if isinstance(v, V) else v.data_ptr())


def L(v):
    return 0 if v is None else v.ld


class Run(object):
    """one case: deterministic inputs, the calls it makes, its outputs"""
    def __init__(self, dtype, device=None):
        self.dtype = dtype
        self.code = nv.BF16 if dtype == 'bf16' else nv.F32
        self.td = torch.bfloat16 if dtype == 'bf16' else torch.float32
        self.dev = torch.device(device or DEVICE)
        self.seed = 1000
        self.entries = []

    def rnd(self, shape, lo=-8, hi=8, q=4.0):
        self.seed += 1
        return torch.randint(lo, hi + 1, tuple(shape), generator=torch.Generator().manual_seed(self.seed)).float() / q

    def f32(self, shape, lo=-8, hi=8, q=4.0):
        return self.rnd(shape, lo, hi, q).to(self.dev)

    def full(self, shape, value, dtype=torch.float32):
        return torch.full(tuple(shape), value, dtype=dtype, device=self.dev)

    def view(self, N, H, W, Cp, C=None, fill=True):
        buf = torch.full((N * H * W, Cp + 8), SENTINEL, dtype=self.td, device=self.dev)
        if fill:
            v = self.rnd((N * H * W, Cp))
            if C is not None and C < Cp:
                v[:, C:] = 0
            buf[:, :Cp] = v.to(self.dev, self.td)
        return V(buf, Cp + 8)

    def coef(self, C, Cp):
        c = torch.zeros(4, Cp)
        c[0, :C], c[1, :C] = self.rnd((C,), 1, 3, 2.0), self.rnd((C,))          # scale, shift
        c[2, :C], c[3, :C] = self.rnd((C,)), self.rnd((C,), 1, 4, 2.0)          # mean, invstd
        return c.to(self.dev)

    def bcoef(self, C, Cp):
        c = torch.zeros(3, Cp)
        c[0, :C], c[1, :C], c[2, :C] = self.rnd((C,), 1, 3, 2.0), self.rnd((C,)), self.rnd((C,))
        return c.to(self.dev)

    def drop(self, N, Cp, on):
        return self.f32((N, Cp), 0, 1, 0.5) if on else None                     # Dropout2d table: 0 or 2

    def table(self, C, Cp, count, ld=None):
        """[16][2][ld] replicated sums whose mean and variance are multiples of 1/4; the padding holds a sentinel"""
        ld = ld or Cp
        t = torch.zeros(16, 2, ld, dtype=torch.float64)
        if ld > Cp:
            t[:, :, Cp:] = SENTINEL
        mu, var = self.rnd((C,)).double(), self.rnd((C,), 2, 16).double()
        t[3, 0, :C] = count * mu
        t[11, 1, :C] = count * (mu * mu + var)
        return t.to(self.dev)

    def call(self, name, *args):
        self.entries.append(name)
        nv.call(name, *args)                # (raises with the library's message on a non-zero status)


def _sha(t):
    t = t.detach().contiguous().cpu()
    t = t.view(torch.int16) if t.dtype == torch.bfloat16 else t
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def _outs(**kw):
    return {k: (v.buf if isinstance(v, V) else v) for k, v in kw.items() if v is not None}


def _bn_params(r, C, Cp):
    """gamma, beta, running mean, running variance, batch counter"""
    return (r.f32((C,), 2, 6), r.f32((C,)), r.f32((C,)), r.f32((C,), 1, 8), torch.full((1,), 3, dtype=torch.int64, device=r.dev))


# ------------------------------------------------------------------------------------------------ forward
def row_fwd(r, s, pool, res):
    N, H, W, C, act, _, up, drop = s
    Cp = pad8(C)
    y, coef, dm = r.view(N, H, W, Cp, C), r.coef(C, Cp), r.drop(N, Cp, drop)
    out = r.view(N, H, W, Cp, fill=False)
    po = r.view(N, H // 2, W // 2, Cp, fill=False) if pool else None
    uo = r.view(N, 2 * H, 2 * W, Cp, fill=False) if up else None
    rs = r.view(N, H, W, Cp, C) if res else None
    r.call('segnb_bn_act_fwd', r.code, y.ptr, y.ld, N, H, W, Cp, P(coef), act, SLOPE, P(dm), out.ptr, out.ld, P(po), L(po),
           P(uo), L(uo), P(rs), L(rs), None)
    return _outs(out=out, pool_out=po, up_out=uo)


def row_fwd_stats(r, s):
    N, H, W, C, act, _, _, drop = s
    Cp = pad8(C)
    y, coef, dm, out = r.view(N, H, W, Cp, C), r.coef(C, Cp), r.drop(N, Cp, drop), r.view(N, H, W, Cp, fill=False)
    st = r.full((16, 2, Cp + 16), 0.0, torch.float64)
    r.call('segnb_bn_act_fwd_stats', r.code, y.ptr, y.ld, N, H, W, Cp, P(coef), act, SLOPE, P(dm), out.ptr, out.ld, P(st), Cp + 16,
           None)
    return _outs(out=out, out_stats=st)


def row_fused(r, s, kind, K=0):
    """segnb_bn_fwd_fused (pooling / upsampling as the shape says; kind 'res': with a residual input), _ld, _head"""
    N, H, W, C, act, pool, up, drop = s
    Cp = pad8(C)
    y, dm = r.view(N, H, W, Cp, C), r.drop(N, Cp, drop)
    gamma, beta, rm, rv, nbt = _bn_params(r, C, Cp)
    coef, clear = r.full((4, Cp), SENTINEL), r.full((16, 2, Cp), SENTINEL, torch.float64)
    out = r.view(N, H, W, Cp, fill=False)
    head = (y.ptr, y.ld, N, H, W, C, Cp)
    bn = (P(gamma), P(beta), EPS, MOM, P(rm), P(rv), P(nbt), P(coef), P(clear), act, SLOPE, P(dm), out.ptr, out.ld)
    po = uo = logits = None
    if kind == 'ld':
        st = r.table(C, Cp, N * H * W, Cp + 16)
        r.call('segnb_bn_fwd_fused_ld', r.code, *head, P(st), Cp + 16, *bn, None)
    elif kind == 'head':
        st, hw, hb = r.table(C, Cp, N * H * W), r.f32((K, C)), r.f32((K,))
        logits = r.full((N, K, H, W), SENTINEL)
        r.call('segnb_bn_fwd_fused_head', r.code, *head, P(st), *bn, P(hw), P(hb), K, P(logits), None)
    else:
        st = r.table(C, Cp, N * H * W)
        po = r.view(N, H // 2, W // 2, Cp, fill=False) if pool else None
        uo = r.view(N, 2 * H, 2 * W, Cp, fill=False) if up else None
        rs = r.view(N, H, W, Cp, C) if kind == 'res' else None
        r.call('segnb_bn_fwd_fused', r.code, *head, P(st), *bn, P(po), L(po), P(uo), L(uo), P(rs), L(rs), None)
    return _outs(out=out, pool_out=po, up_out=uo, logits=logits, coef=coef, running_mean=rm, running_var=rv, nbt=nbt,
                 cleared=clear, stats_in=st)


# ------------------------------------------------------------------------------------------------ backward: reduction
def _sources(r, s, src):
    """the gradient sources of set `src` (bit 0 direct, bit 1 pooled, bit 2 upsampled)"""
    N, H, W, C = s[:4]
    Cp = pad8(C)
    gd = r.view(N, H, W, Cp, C) if src & 1 else None
    gp = r.view(N, H // 2, W // 2, Cp, C) if src & 2 else None
    gu = r.view(N, 2 * H, 2 * W, Cp, C) if src & 4 else None
    return gd, gp, gu


def row_reduce(r, s, src, res=False, store=True):
    N, H, W, C, act, _, _, drop = s
    Cp = pad8(C)
    y, coef, dm = r.view(N, H, W, Cp, C), r.coef(C, Cp), r.drop(N, Cp, drop)
    gd, gp, gu = _sources(r, s, src)
    dz = r.view(N, H, W, Cp, fill=False) if store else None
    rs = r.view(N, H, W, Cp, C) if res else None
    sums = r.full((16, 2, Cp), 0.0, torch.float64)
    r.call('segnb_bn_act_bwd_reduce', r.code, y.ptr, y.ld, N, H, W, Cp, P(coef), act, SLOPE, P(dm), P(gd), L(gd), P(gp), L(gp),
           P(gu), L(gu), P(dz), L(dz), P(sums), P(rs), L(rs), None)
    return _outs(dz=dz, sums=sums)


def row_reduce_add(r, s, res):
    N, H, W, C, act, _, _, drop = s
    Cp = pad8(C)
    y, coef, dm = r.view(N, H, W, Cp, C), r.coef(C, Cp), r.drop(N, Cp, drop)
    gd, ga, dz = r.view(N, H, W, Cp, C), r.view(N, H, W, Cp, C), r.view(N, H, W, Cp, fill=False)
    rs = r.view(N, H, W, Cp, C) if res else None
    sums = r.full((16, 2, Cp), 0.0, torch.float64)
    r.call('segnb_bn_act_bwd_reduce_add', r.code, y.ptr, y.ld, N, H, W, Cp, P(coef), act, SLOPE, P(dm), gd.ptr, gd.ld, ga.ptr, ga.ld,
           dz.ptr, dz.ld, P(sums), P(rs), L(rs), None)
    return _outs(dz=dz, sums=sums)


def row_head_bn_bwd(r, s, K):
    N, H, W, C, act, _, _, drop = s
    Cp = pad8(C)
    y, coef, dm, dz = r.view(N, H, W, Cp, C), r.coef(C, Cp), r.drop(N, Cp, drop), r.view(N, H, W, Cp, fill=False)
    hw, dl = r.f32((K, C)), r.f32((N, K, H, W))
    sums, dw, db = r.full((16, 2, Cp), 0.0, torch.float64), r.full((K, C), SENTINEL), r.full((K,), SENTINEL)
    r.call('segnb_head_bn_bwd', r.code, y.ptr, y.ld, N, H, W, C, Cp, P(coef), act, SLOPE, P(dm), P(hw), K, P(dl), dz.ptr, dz.ld,
           P(sums), P(dw), P(db), None)
    return _outs(dz=dz, sums=sums, dw=dw, db=db)


# ------------------------------------------------------------------------------------------------ backward: apply
def _fused_bwd(r, s):
    """the arguments every fused apply shares, and the tables it writes"""
    N, H, W, C = s[:4]
    Cp = pad8(C)
    y, coef, sums = r.view(N, H, W, Cp, C), r.coef(C, Cp), r.table(C, Cp, N * H * W)
    gamma, bcoef, dgam, dbet = r.f32((C,), 2, 6), r.full((3, Cp), SENTINEL), r.f32((C,)), r.f32((C,))
    clear = r.full((16, 2, Cp), SENTINEL, torch.float64)
    args = (r.code, y.ptr, y.ld, N, H, W, C, Cp, P(coef), P(sums), P(gamma), P(bcoef), P(dgam), P(dbet), 1, P(clear))
    # (the inputs ride along: they stay alive until the launch has run, and a launch that wrote one of them would show)
    return args, dict(bcoef=bcoef, dgamma=dgam, dbeta=dbet, cleared=clear, y_in=y, coef_in=coef, sums_in=sums, gamma_in=gamma)


def row_apply(r, s, form, src=1, K=0):
    N, H, W, C, act, _, _, drop = s
    Cp = pad8(C)
    acc = form.endswith('_acc')
    dy = r.view(N, H, W, Cp, C, fill=acc)
    if form in ('segnb_bn_bwd_apply', 'segnb_bn_bwd_apply_direct'):
        y, coef, bcoef, g, dbias = r.view(N, H, W, Cp, C), r.coef(C, Cp), r.bcoef(C, Cp), r.view(N, H, W, Cp, C), r.full((C,), 0.0)
        if form == 'segnb_bn_bwd_apply':
            r.call(form, r.code, y.ptr, y.ld, N, H, W, Cp, P(coef), P(bcoef), g.ptr, g.ld, dy.ptr, dy.ld, P(dbias), C, None)
        else:
            r.call(form, r.code, y.ptr, y.ld, N, H, W, Cp, P(coef), P(bcoef), act, SLOPE, g.ptr, g.ld, dy.ptr, dy.ld, P(dbias), C,
                   None)
        return _outs(dy=dy, dbias=dbias)
    args, tables = _fused_bwd(r, s)
    if form in ('segnb_bn_bwd_apply_fused', 'segnb_bn_bwd_apply_fused_acc'):
        dz = r.view(N, H, W, Cp, C)
        r.call(form, *args, dz.ptr, dz.ld, dy.ptr, dy.ld, None)
    elif form in ('segnb_bn_bwd_apply_fused_direct', 'segnb_bn_bwd_apply_fused_direct_acc'):
        g = r.view(N, H, W, Cp, C)
        r.call(form, *args, act, SLOPE, g.ptr, g.ld, dy.ptr, dy.ld, None)
    elif form == 'segnb_bn_bwd_apply_fused_src':
        dm = r.drop(N, Cp, drop)
        gd, gp, gu = _sources(r, s, src)
        r.call(form, *args, act, SLOPE, P(dm), P(gd), L(gd), P(gp), L(gp), P(gu), L(gu), dy.ptr, dy.ld, None)
    else:
        assert form == 'segnb_head_bn_bwd_apply'
        dm, hw, dl = r.drop(N, Cp, drop), r.f32((K, C)), r.f32((N, K, H, W))
        r.call(form, *args, act, SLOPE, P(dm), P(hw), K, P(dl), dy.ptr, dy.ld, None)
    return _outs(dy=dy, **tables)


# ------------------------------------------------------------------------------------------------ per-channel launches
def row_finalize(r, s, form):
    N, H, W, C = s[:4]
    Cp, count = pad8(C), float(N * H * W)
    gamma, beta, rm, rv, nbt = _bn_params(r, C, Cp)
    st, coef = r.table(C, Cp, count), r.full((4, Cp), SENTINEL)
    if form == 'keep':
        clear = r.full((16, 2, Cp), SENTINEL, torch.float64)
        r.call('segnb_bn_finalize_keep', P(st), C, Cp, count, P(gamma), P(beta), EPS, MOM, P(rm), P(rv), P(nbt), P(coef), P(clear), None)
        return _outs(coef=coef, running_mean=rm, running_var=rv, nbt=nbt, stats_in=st, cleared=clear)
    r.call('segnb_bn_finalize', P(st), C, Cp, count, P(gamma), P(beta), EPS, MOM, P(rm), P(rv), P(nbt), 1 if form == 'train' else 0,
           P(coef), None)
    return _outs(coef=coef, running_mean=rm, running_var=rv, nbt=nbt, stats_in=st)


def row_bwd_finalize(r, s, clear):
    N, H, W, C = s[:4]
    Cp, count = pad8(C), float(N * H * W)
    sums, coef, gamma = r.table(C, Cp, count), r.coef(C, Cp), r.f32((C,), 2, 6)
    bcoef, dgam, dbet = r.full((3, Cp), SENTINEL), r.f32((C,)), r.f32((C,))
    if clear:
        cl = r.full((16, 2, Cp), SENTINEL, torch.float64)
        r.call('segnb_bn_bwd_finalize_clear', P(sums), C, Cp, count, P(gamma), P(coef), P(bcoef), P(dgam), P(dbet), 1, P(cl), None)
        return _outs(bcoef=bcoef, dgamma=dgam, dbeta=dbet, sums_in=sums, cleared=cl)
    r.call('segnb_bn_bwd_finalize', P(sums), C, Cp, count, P(gamma), P(coef), P(bcoef), P(dgam), P(dbet), 0, None)
    return _outs(bcoef=bcoef, dgamma=dgam, dbeta=dbet, sums_in=sums)


class BiasGradJob(ctypes.Structure):
    _fields_ = [('sums', ctypes.c_void_p), ('gb', ctypes.c_void_p), ('C', ctypes.c_int), ('Cp', ctypes.c_int)]


def row_bias_grad_multi(r, s):
    C = s[3]
    Cp = pad8(C)
    assert nv.query('segnb_bias_grad_job_bytes') == ctypes.sizeof(BiasGradJob)
    sums = [r.table(C, Cp, 64.0), r.table(C, Cp, 16.0)]
    gb = r.f32((C,))
    jobs = (BiasGradJob * 2)(BiasGradJob(P(sums[0]), P(gb), C, Cp), BiasGradJob(P(sums[1]), None, C, Cp))
    dev_jobs = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(r.dev)
    r.call('segnb_bias_grad_multi', P(dev_jobs), 2, None)
    return _outs(gb=gb, sums0=sums[0], sums1=sums[1])


def row_stats(r, s, ld):
    N, H, W, C = s[:4]
    Cp = pad8(C)
    x = r.view(N, H, W, Cp, C)
    if ld:
        st = r.full((16, 2, Cp + 16), 0.0, torch.float64)
        r.call('segnb_bn_stats_ld', r.code, x.ptr, x.ld, N, H, W, Cp, P(st), Cp + 16, None)
    else:
        st = r.full((16, 2, Cp), 0.0, torch.float64)
        r.call('segnb_bn_stats', r.code, x.ptr, x.ld, N, H, W, Cp, P(st), None)
    return _outs(stats=st)


def row_abn(r, s):
    C = s[3]
    w, scale, dscale, dw = r.f32((C,)), r.full((C,), SENTINEL), r.f32((C,)), r.f32((C,))
    r.call('segnb_abn_scale', P(w), 0.25, P(scale), C, None)
    r.call('segnb_abn_dscale', P(w), P(dscale), P(dw), C, None)
    return _outs(scale=scale, dscale=dscale, dw=dw)


# ------------------------------------------------------------------------------------------------ classifier heads
HEAD_GEOM = (2, 6, 10)          # N, H, W of the head rows


def row_head(r, C, K):
    N, H, W = HEAD_GEOM
    Cp = pad8(C)
    a, w, b = r.view(N, H, W, Cp, C), r.f32((K, C)), r.f32((K,))
    logits = r.full((N, K, H, W), SENTINEL)
    r.call('segnb_head_fwd', r.code, a.ptr, a.ld, N, H, W, C, P(w), P(b), K, P(logits), None)
    return _outs(logits=logits)


def row_head_bwd(r, C, K):
    N, H, W = HEAD_GEOM
    Cp = pad8(C)
    a, w, dl = r.view(N, H, W, Cp, C), r.f32((K, C)), r.f32((N, K, H, W))
    da, dw, db = r.view(N, H, W, Cp, fill=False), r.full((K, C), SENTINEL), r.full((K,), SENTINEL)
    r.call('segnb_head_bwd', r.code, a.ptr, a.ld, N, H, W, C, Cp, P(w), K, P(dl), da.ptr, da.ld, P(dw), P(db), None)
    return _outs(da=da, dw=dw, db=db)


def row_head_conv(r, C, K, kh, kw, pad, act):
    N, H, W = 2, 9, 11
    Cp = pad8(C)
    Ho, Wo = H + 2 * pad - kh + 1, W + 2 * pad - kw + 1
    assert nv.query('segnb_head_conv_ok', C, K, kh, kw)
    a, w, b = r.view(N, H, W, Cp, C), r.f32((K, C, kh, kw)), r.f32((K,))
    logits = r.full((N, K, Ho, Wo), SENTINEL)
    r.call('segnb_head_conv_fwd', r.code, a.ptr, a.ld, N, H, W, C, P(w), kh, kw, pad, P(b), K, P(logits), None)
    dl, da = r.f32((N, K, Ho, Wo)), r.view(N, H, W, Cp, fill=False)
    dw, db = r.full((K, C, kh, kw), SENTINEL), r.full((K,), SENTINEL)
    sums = r.full((16, 2, Cp), 0.0, torch.float64) if act >= 0 else None
    r.call('segnb_head_conv_bwd', r.code, a.ptr, a.ld, N, H, W, C, Cp, P(w), kh, kw, pad, K, P(dl), act, SLOPE, da.ptr, da.ld,
           P(dw), P(db), P(sums), None)
    return _outs(logits=logits, da=da, dw=dw, db=db, sums=sums)


# ------------------------------------------------------------------------------------------------ what left norm_act.hip
def row_add(r, s, operands):
    N, H, W, C = s[:4]
    Cp = pad8(C)
    a = r.view(N, H, W, Cp, C) if operands & 1 else None
    b = r.view(N, H, W, Cp, C) if operands & 2 else None
    out = r.view(N, H, W, Cp, fill=False)
    r.call('segnb_add', r.code, P(a), L(a), P(b), L(b), out.ptr, out.ld, N, H, W, Cp, None)
    return _outs(out=out)


def row_maxpool(r, s, k, st, pd, form):
    """forward (with the argmax positions unless form is 'scan'), then the backward of the form"""
    N, H, W, C = s[:4]
    Cp = pad8(C)
    Ho, Wo = (H + 2 * pd - k) // st + 1, (W + 2 * pd - k) // st + 1
    x, out = r.view(N, H, W, Cp, C), r.view(N, Ho, Wo, Cp, fill=False)
    idx = None if form == 'scan' else torch.full((N * Ho * Wo * Cp,), 99, dtype=torch.uint8, device=r.dev)
    r.call('segnb_maxpool_fwd', r.code, x.ptr, x.ld, N, H, W, Cp, k, st, pd, out.ptr, out.ld, P(idx), None)
    go, dx = r.view(N, Ho, Wo, Cp, C), r.view(N, H, W, Cp, fill=False)
    if form == 'add':
        go2 = r.view(N, Ho, Wo, Cp, C)
        r.call('segnb_maxpool_bwd_add', r.code, x.ptr, x.ld, go.ptr, go.ld, go2.ptr, go2.ld, N, H, W, Cp, k, st, pd, dx.ptr, dx.ld,
               P(idx), None)
    else:
        r.call('segnb_maxpool_bwd', r.code, x.ptr, x.ld, go.ptr, go.ld, N, H, W, Cp, k, st, pd, dx.ptr, dx.ld, P(idx), None)
    return _outs(out=out, idx=idx, dx=dx)


def row_upsample(r, s):
    N, H, W, C = s[:4]
    Cp = pad8(C)
    x, out = r.view(N, H, W, Cp, C), r.view(N, 2 * H, 2 * W, Cp, fill=False)
    r.call('segnb_upsample_bilinear2x_fwd', r.code, x.ptr, x.ld, N, H, W, Cp, out.ptr, out.ld, None)
    go, dx = r.view(N, 2 * H, 2 * W, Cp, C), r.view(N, H, W, Cp, fill=False)
    r.call('segnb_upsample_bilinear2x_bwd', r.code, go.ptr, go.ld, N, H, W, Cp, dx.ptr, dx.ld, None)
    return _outs(out=out, dx=dx)


def row_nchw(r, s):
    N, H, W, C = s[:4]
    a, out = r.view(N, H, W, pad8(C), C), r.full((N, C, H, W), SENTINEL)
    r.call('segnb_nhwc_to_nchw_f32', r.code, a.ptr, a.ld, N, H, W, C, P(out), None)
    return _outs(out=out)


def row_optim(r, name):
    n = 4099                    # not a multiple of 4: the scalar tail of sgd_kernel
    p, g = r.f32((n,)), r.f32((n,))
    if name == 'sgd':
        r.call('segnb_sgd_step', P(p), P(g), n, 0.25, None)
        return _outs(p=p)
    if name == 'rmsprop':
        sq = r.f32((n,), 0, 8)
        r.call('segnb_rmsprop_step', P(p), P(g), P(sq), n, 0.25, 0.75, 0.125, None)
        return _outs(p=p, square_avg=sq)
    m, v = r.f32((n,)), r.f32((n,), 0, 8)
    r.call('segnb_adam_step', P(p), P(g), P(m), P(v), n, 0.25, 0.75, 0.875, 0.125, 3, None)
    return _outs(p=p, exp_avg=m, exp_avg_sq=v)


def row_pack(r, what):
    N, C, H, W, Cp = 2, 3, 5, 7, 8
    out = r.view(N, H, W, Cp, fill=False)
    if what == 'nchw':
        x = r.f32((N, C, H, W))
        r.call('segnb_pack_input_nchw', P(x), N, C, H, W, out.ptr, r.code, Cp, out.ld, None)
    elif what == 'u8':
        r.seed += 1
        img = torch.randint(0, 256, (N, H, W, C), generator=torch.Generator().manual_seed(r.seed)).to(torch.uint8).to(r.dev)
        r.call('segnb_pack_input_u8', P(img), N, H, W, C, 0.25, nv.float_array([0.5, 1.0, 1.5]), nv.float_array([0.5, 2.0, 4.0]),
               out.ptr, r.code, Cp, out.ld, None)
    else:
        M, Ci, T = 6, 5, 3
        w = r.f32((M, Ci, T))
        mmap = torch.tensor(list(range(M)) + [-1, -1], dtype=torch.int32, device=r.dev)
        cmap = torch.tensor(list(range(Ci)) + [-1, -1, -1], dtype=torch.int32, device=r.dev)
        out = torch.full((8 * T * 8 + 8,), SENTINEL, dtype=r.td, device=r.dev)
        r.call('segnb_pack_weight', P(w), P(out), r.code, 8, 8, T, Ci * T, T, nv.int_array([0, 1, 2]), P(mmap), P(cmap), None)
    return _outs(out=out)


# ------------------------------------------------------------------------------------------------ the rows
def _rows():
    """{row id: (function, arguments after the Run)}: one row per branch of a host-side dispatch, per shape where the shape
    changes the launch; every row runs in both dtypes"""
    rows = {}
    for i, s in enumerate(SHAPES):
        t = 's%d' % i
        for pool in (False, True):
            for res in (False, True):
                rows['fwd%s%s/%s' % ('_pool' if pool else '', '_res' if res else '', t)] = (row_fwd, (s, pool, res))
        rows['fwd_stats/' + t] = (row_fwd_stats, (s,))
        rows['fused/' + t] = (row_fused, (s, 'plain'))
        if not s[5]:
            rows['fused_res/' + t] = (row_fused, (s, 'res'))
        rows['fused_ld/' + t] = (row_fused, (s, 'ld'))
        for src in range(1, 8):
            rows['reduce_src%d/%s' % (src, t)] = (row_reduce, (s, src))
            rows['apply_fused_src%d/%s' % (src, t)] = (row_apply, (s, 'segnb_bn_bwd_apply_fused_src', src))
        for src in (1, 4, 5):
            rows['reduce_src%d_res/%s' % (src, t)] = (row_reduce, (s, src, True))
        for src in (1, 3):
            rows['reduce_src%d_nodz/%s' % (src, t)] = (row_reduce, (s, src, False, False))
        rows['reduce_add/' + t] = (row_reduce_add, (s, False))
        rows['reduce_add_res/' + t] = (row_reduce_add, (s, True))
        for form in ('segnb_bn_bwd_apply', 'segnb_bn_bwd_apply_direct', 'segnb_bn_bwd_apply_fused', 'segnb_bn_bwd_apply_fused_acc',
                     'segnb_bn_bwd_apply_fused_direct', 'segnb_bn_bwd_apply_fused_direct_acc'):
            rows['%s/%s' % (form[len('segnb_bn_bwd_'):], t)] = (row_apply, (s, form))
        for form in ('train', 'eval', 'keep'):
            rows['finalize_%s/%s' % (form, t)] = (row_finalize, (s, form))
        rows['bwd_finalize/' + t] = (row_bwd_finalize, (s, False))
        rows['bwd_finalize_clear/' + t] = (row_bwd_finalize, (s, True))
        rows['stats/' + t] = (row_stats, (s, False))
        rows['stats_ld/' + t] = (row_stats, (s, True))
        rows['add/' + t] = (row_add, (s, 3))
        rows['upsample/' + t] = (row_upsample, (s,))
        rows['nchw/' + t] = (row_nchw, (s,))
        for form in ('idx', 'scan', 'add'):
            rows['maxpool3s2_%s/%s' % (form, t)] = (row_maxpool, (s, 3, 2, 1, form))
    for i in HEAD_SHAPES:
        for K in (1, 3):
            rows['fused_head_k%d/s%d' % (K, i)] = (row_fused, (SHAPES[i], 'head', K))
            rows['head_bn_bwd_k%d/s%d' % (K, i)] = (row_head_bn_bwd, (SHAPES[i], K))
            rows['head_bn_bwd_apply_k%d/s%d' % (K, i)] = (row_apply, (SHAPES[i], 'segnb_head_bn_bwd_apply', 1, K))
    rows['add_copy/s1'] = (row_add, (SHAPES[1], 1))
    rows['maxpool2s2_idx/s1'] = (row_maxpool, (SHAPES[1], 2, 2, 0, 'idx'))
    rows['maxpool2s2_scan/s1'] = (row_maxpool, (SHAPES[1], 2, 2, 0, 'scan'))
    rows['bias_grad_multi/s1'] = (row_bias_grad_multi, (SHAPES[1],))
    rows['abn/s1'] = (row_abn, (SHAPES[1],))
    for C in (32, 96, 20):      # narrow, wide (the chunk-per-lane forward), padded channels
        for K in (1, 3, 12, 20):
            rows['head_fwd_c%d_k%d' % (C, K)] = (row_head, (C, K))
        for K in (1, 3, 12):
            rows['head_bwd_c%d_k%d' % (C, K)] = (row_head_bwd, (C, K))
    for C in (32, 20):
        for K, kh, kw, pad in ((1, 1, 1, 0), (1, 2, 2, 1), (1, 2, 4, 1), (2, 2, 2, 0), (3, 1, 1, 0)):
            for act in (-1, nv.ACT_RELU):
                rows['head_conv_c%d_k%d_%dx%d_act%d' % (C, K, kh, kw, act)] = (row_head_conv, (C, K, kh, kw, pad, act))
    for name in ('sgd', 'rmsprop', 'adam'):
        rows['optim_' + name] = (row_optim, (name,))
    for what in ('nchw', 'u8', 'weight'):
        rows['pack_' + what] = (row_pack, (what,))
    return rows


ROWS = _rows()
F32_ONLY = ('bias_grad_multi/', 'abn/', 'optim_', 'finalize_', 'bwd_finalize')      # no dtype argument: one case
CASES = sorted('%s:%s' % (row, dt) for row in ROWS for dt in DTYPES if dt == 'f32' or not row.startswith(F32_ONLY))


def run_outputs(case, device=None):
    """the output buffers themselves, on the device they were written on (tests/ew_oracle.py compares them with a float64
    oracle; run_case digests them) -> {output: tensor}"""
    row, dt = case.rsplit(':', 1)
    fn, args = ROWS[row]
    r = Run(dt, device)
    outs = fn(r, *args)
    if r.dev.type == 'cuda':
        torch.cuda.synchronize()
    return outs


def run_case(case, device=None):
    """-> {'entries': the entry points called, 'sha': {output: SHA-256 of the whole buffer}, 'excluded': {output: reason}}"""
    row, dt = case.rsplit(':', 1)
    fn, args = ROWS[row]
    r = Run(dt, device)
    outs = fn(r, *args)
    if r.dev.type == 'cuda':
        torch.cuda.synchronize()
    excluded = {k: why for (rw, k), why in EXCLUDED.items() if rw == row}
    return {'entries': sorted(set(r.entries)), 'sha': {k: _sha(v) for k, v in sorted(outs.items()) if k not in excluded},
            'excluded': excluded}


# ------------------------------------------------------------------------------------------------ refusals
def _refusal_calls():
    """{name: (entry point, arguments)}: every call is refused by a host-side check before anything touches the device, so the
    pointers are never followed.  Where a call trips two checks the first one's message is the one recorded."""
    X = 0x1000                  # a non-NULL pointer
    BAD = 7                     # no such dtype
    N, H, W, C, Cp, ld = 2, 8, 8, 30, 32, 40
    geo, geoc = (N, H, W, Cp), (N, H, W, C, Cp)
    bnp = (X, X, EPS, MOM, X, X, X, X, X, 1, SLOPE, None)          # gamma .. dropmul of the fused forwards

    def fwd(dt=nv.BF16, y=X, g=geo, out=X, pool=None, res=None):
        return ('segnb_bn_act_fwd', (dt, y, ld, *g, X, 1, SLOPE, None, out, ld, pool, ld, None, 0, res, ld, None))

    def reduce(dt=nv.BF16, g=geo, gd=X, gp=None, dz=X, sums=X, res=None):
        return ('segnb_bn_act_bwd_reduce', (dt, X, ld, *g, X, 1, SLOPE, None, gd, ld, gp, ld, None, 0, dz, ld, sums, res, ld, None))

    def fused_apply(name, dt=nv.BF16, sums=X, tail=()):
        return (name, (dt, X, ld, *geoc, X, sums, X, X, X, X, 0, None) + tail + (None,))

    def maxpool_bwd(dt=nv.BF16, idx=X, x=X):
        return ('segnb_maxpool_bwd', (dt, x, ld, X, ld, N, H, W, Cp, 3, 2, 1, X, ld, idx, None))

    def head_conv_bwd(dt=nv.BF16, Cp_=Cp, C_=C, K=1, a=X):
        return ('segnb_head_conv_bwd', (dt, a, Cp_ + 8, N, H, W, C_, Cp_, X, 2, 2, 1, K, X, -1, SLOPE, X, Cp_ + 8, X, X, None, None))

    calls = {
        # ---- an unknown dtype at every entry point that takes one
        'dtype/segnb_bn_act_fwd': fwd(BAD),
        'dtype/segnb_bn_act_fwd_pool_res': fwd(BAD, pool=X, res=X),
        'dtype/segnb_bn_act_fwd_stats': ('segnb_bn_act_fwd_stats', (BAD, X, ld, *geo, X, 1, SLOPE, None, X, ld, X, Cp, None)),
        'dtype/segnb_bn_fwd_fused': ('segnb_bn_fwd_fused', (BAD, X, ld, *geoc, X, *bnp, X, ld, None, 0, None, 0, None, 0, None)),
        'dtype/segnb_bn_fwd_fused_ld': ('segnb_bn_fwd_fused_ld', (BAD, X, ld, *geoc, X, Cp, *bnp, X, ld, None)),
        'dtype/segnb_bn_fwd_fused_head': ('segnb_bn_fwd_fused_head', (BAD, X, ld, *geoc, X, *bnp, X, ld, X, X, 3, X, None)),
        'dtype/segnb_bn_act_bwd_reduce': reduce(BAD),
        'dtype/segnb_bn_act_bwd_reduce_add': ('segnb_bn_act_bwd_reduce_add',
                                              (BAD, X, ld, *geo, X, 1, SLOPE, None, X, ld, X, ld, X, ld, X, None, 0, None)),
        'dtype/segnb_head_bn_bwd_apply': fused_apply('segnb_head_bn_bwd_apply', BAD, tail=(1, SLOPE, None, X, 3, X, X, ld)),
        'dtype/segnb_bn_bwd_apply': ('segnb_bn_bwd_apply', (BAD, X, ld, *geo, X, X, X, ld, X, ld, None, C, None)),
        'dtype/segnb_bn_bwd_apply_direct': ('segnb_bn_bwd_apply_direct', (BAD, X, ld, *geo, X, X, 1, SLOPE, X, ld, X, ld, None, C, None)),
        'dtype/segnb_bn_bwd_apply_fused': fused_apply('segnb_bn_bwd_apply_fused', BAD, tail=(X, ld, X + 64, ld)),
        'dtype/segnb_bn_bwd_apply_fused_acc': fused_apply('segnb_bn_bwd_apply_fused_acc', BAD, tail=(X, ld, X + 64, ld)),
        'dtype/segnb_bn_bwd_apply_fused_direct': fused_apply('segnb_bn_bwd_apply_fused_direct', BAD, tail=(1, SLOPE, X, ld, X + 64, ld)),
        'dtype/segnb_bn_bwd_apply_fused_direct_acc': fused_apply('segnb_bn_bwd_apply_fused_direct_acc', BAD,
                                                                 tail=(1, SLOPE, X, ld, X + 64, ld)),
        'dtype/segnb_bn_bwd_apply_fused_src': fused_apply('segnb_bn_bwd_apply_fused_src', BAD,
                                                          tail=(1, SLOPE, None, X, ld, None, 0, None, 0, X + 64, ld)),
        'dtype/segnb_bn_stats': ('segnb_bn_stats', (BAD, X, ld, *geo, X, None)),
        'dtype/segnb_bn_stats_ld': ('segnb_bn_stats_ld', (BAD, X, ld, *geo, X, Cp, None)),
        'dtype/segnb_add': ('segnb_add', (BAD, X, ld, X, ld, X, ld, *geo, None)),
        'dtype/segnb_maxpool_fwd': ('segnb_maxpool_fwd', (BAD, X, ld, *geo, 3, 2, 1, X, ld, None, None)),
        'dtype/segnb_maxpool_bwd_idx': maxpool_bwd(BAD),
        'dtype/segnb_maxpool_bwd_scan': maxpool_bwd(BAD, idx=None),
        'dtype/segnb_maxpool_bwd_add': ('segnb_maxpool_bwd_add', (BAD, X, ld, X, ld, X, ld, N, H, W, Cp, 3, 2, 1, X, ld, X, None)),
        'dtype/segnb_upsample_bilinear2x_fwd': ('segnb_upsample_bilinear2x_fwd', (BAD, X, ld, *geo, X, ld, None)),
        'dtype/segnb_upsample_bilinear2x_bwd': ('segnb_upsample_bilinear2x_bwd', (BAD, X, ld, *geo, X, ld, None)),
        'dtype/segnb_nhwc_to_nchw_f32': ('segnb_nhwc_to_nchw_f32', (BAD, X, ld, N, H, W, C, X, None)),
        'dtype/segnb_head_fwd_narrow': ('segnb_head_fwd', (BAD, X, ld, N, H, W, C, X, X, 3, X, None)),
        'dtype/segnb_head_fwd_narrow_k12': ('segnb_head_fwd', (BAD, X, ld, N, H, W, C, X, X, 12, X, None)),
        'dtype/segnb_head_fwd_wide': ('segnb_head_fwd', (BAD, X, 104, N, H, W, 96, X, X, 3, X, None)),
        'dtype/segnb_head_bwd': ('segnb_head_bwd', (BAD, X, ld, *geoc, X, 3, X, X, ld, X, X, None)),
        'dtype/segnb_head_conv_fwd': ('segnb_head_conv_fwd', (BAD, X, ld, N, H, W, C, X, 2, 2, 1, X, 1, X, None)),
        'dtype/segnb_head_conv_bwd': head_conv_bwd(BAD),
        'dtype/segnb_pack_input_nchw': ('segnb_pack_input_nchw', (X, N, 3, H, W, X, BAD, 8, 16, None)),
        'dtype/segnb_pack_input_u8': ('segnb_pack_input_u8', (X, N, H, W, 3, 0.25, nv.float_array([0.5, 1.0, 1.5]),
                                                              nv.float_array([0.5, 2.0, 4.0]), X, BAD, 8, 16, None)),
        'dtype/segnb_pack_weight': ('segnb_pack_weight', (X, X, BAD, 8, 8, 3, 15, 3, nv.int_array([0, 1, 2]), X, X, None)),
        # ---- Cp % 8 != 0 (check_ew), through each launcher that names itself in the message
        'cp/segnb_bn_act_fwd': fwd(g=(N, H, W, 30)),
        'cp/segnb_bn_act_bwd_reduce': reduce(g=(N, H, W, 30)),
        'cp/segnb_bn_bwd_apply': ('segnb_bn_bwd_apply', (nv.BF16, X, ld, N, H, W, 30, X, X, X, ld, X, ld, None, C, None)),
        'cp/segnb_bn_stats': ('segnb_bn_stats', (nv.BF16, X, ld, N, H, W, 30, X, None)),
        'cp/segnb_add': ('segnb_add', (nv.BF16, X, ld, X, ld, X, ld, N, H, W, 30, None)),
        'cp/segnb_maxpool_bwd': ('segnb_maxpool_bwd', (nv.BF16, X, ld, X, ld, N, H, W, 30, 3, 2, 1, X, ld, X, None)),
        'cp/pixels_exceed_int32': fwd(g=(1 << 10, 1 << 10, 1 << 10, Cp)),
        'cp/both_dtype_and_cp': fwd(BAD, g=(N, H, W, 30)),
        # ---- a NULL tensor, once per distinct message
        'null/launch_bn_act_fwd': fwd(y=None),
        'null/launch_bn_act_fwd_no_output': fwd(out=None),
        'null/segnb_bn_act_fwd_stats': ('segnb_bn_act_fwd_stats', (nv.BF16, X, ld, *geo, X, 1, SLOPE, None, X, ld, None, Cp, None)),
        'null/segnb_bn_act_bwd_reduce': ('segnb_bn_act_bwd_reduce',
                                         (nv.BF16, None, ld, *geo, X, 1, SLOPE, None, X, ld, None, 0, None, 0, X, ld, X, None, 0, None)),
        'null/segnb_bn_act_bwd_reduce_add': ('segnb_bn_act_bwd_reduce_add',
                                             (nv.BF16, X, ld, *geo, X, 1, SLOPE, None, X, ld, None, ld, X, ld, X, None, 0, None)),
        'null/segnb_head_bn_bwd': ('segnb_head_bn_bwd', (nv.BF16, X, ld, *geoc, X, 1, SLOPE, None, None, 3, X, X, ld, X, X, X, None)),
        'null/segnb_head_bn_bwd_apply': fused_apply('segnb_head_bn_bwd_apply', sums=None, tail=(1, SLOPE, None, X, 3, X, X, ld)),
        'null/launch_bn_bwd_apply': ('segnb_bn_bwd_apply', (nv.BF16, X, ld, *geo, X, X, None, ld, X, ld, None, C, None)),
        'null/segnb_bn_bwd_apply_direct': ('segnb_bn_bwd_apply_direct', (nv.BF16, X, ld, *geo, X, X, 1, SLOPE, None, ld, X, ld, None, C, None)),
        'null/segnb_bn_bwd_apply_fused': fused_apply('segnb_bn_bwd_apply_fused', sums=None, tail=(X, ld, X + 64, ld)),
        'null/segnb_bn_bwd_apply_fused_direct': fused_apply('segnb_bn_bwd_apply_fused_direct', tail=(1, SLOPE, None, ld, X + 64, ld)),
        'null/segnb_bn_bwd_apply_fused_src': fused_apply('segnb_bn_bwd_apply_fused_src', sums=None,
                                                         tail=(1, SLOPE, None, X, ld, None, 0, None, 0, X + 64, ld)),
        'null/segnb_bn_fwd_fused': ('segnb_bn_fwd_fused', (nv.BF16, X, ld, *geoc, None, *bnp, X, ld, None, 0, None, 0, None, 0, None)),
        'null/segnb_bn_fwd_fused_head': ('segnb_bn_fwd_fused_head', (nv.BF16, X, ld, *geoc, None, *bnp, X, ld, X, X, 3, X, None)),
        'null/segnb_bn_finalize': ('segnb_bn_finalize', (X, C, Cp, 64.0, X, X, EPS, MOM, X, X, X, 1, None, None)),
        'null/segnb_bn_finalize_source': ('segnb_bn_finalize', (None, C, Cp, 64.0, X, X, EPS, MOM, X, X, X, 1, X, None)),
        'null/segnb_bn_finalize_keep': ('segnb_bn_finalize_keep', (None, C, Cp, 64.0, X, X, EPS, MOM, X, X, X, X, X, None)),
        'null/segnb_bn_bwd_finalize': ('segnb_bn_bwd_finalize', (None, C, Cp, 64.0, X, X, X, X, X, 0, None)),
        'null/segnb_bn_bwd_finalize_clear': ('segnb_bn_bwd_finalize_clear', (X, C, Cp, 64.0, X, None, X, X, X, 0, X, None)),
        'null/segnb_bias_grad_multi': ('segnb_bias_grad_multi', (None, 2, None)),
        'null/launch_bn_stats': ('segnb_bn_stats_ld', (nv.BF16, None, ld, *geo, X, Cp, None)),
        'null/segnb_abn_scale': ('segnb_abn_scale', (None, 0.25, X, C, None)),
        'null/segnb_abn_dscale': ('segnb_abn_dscale', (X, None, X, C, None)),
        'null/segnb_add': ('segnb_add', (nv.BF16, X, ld, X, ld, None, ld, *geo, None)),
        'null/segnb_maxpool_fwd': ('segnb_maxpool_fwd', (nv.BF16, None, ld, *geo, 3, 2, 1, X, ld, None, None)),
        'null/maxpool_bwd_impl': maxpool_bwd(x=None),
        'null/segnb_upsample_bilinear2x_fwd': ('segnb_upsample_bilinear2x_fwd', (nv.BF16, None, ld, *geo, X, ld, None)),
        'null/segnb_upsample_bilinear2x_bwd': ('segnb_upsample_bilinear2x_bwd', (nv.BF16, X, ld, *geo, None, ld, None)),
        'null/segnb_nhwc_to_nchw_f32': ('segnb_nhwc_to_nchw_f32', (nv.BF16, None, ld, N, H, W, C, X, None)),
        'null/segnb_sgd_step': ('segnb_sgd_step', (None, X, 64, 0.25, None)),
        'null/segnb_sgd_step_alignment': ('segnb_sgd_step', (X + 4, X, 64, 0.25, None)),
        'null/segnb_rmsprop_step': ('segnb_rmsprop_step', (X, X, None, 64, 0.25, 0.75, 0.125, None)),
        'null/segnb_adam_step': ('segnb_adam_step', (X, X, X, X, 64, 0.25, 0.75, 0.875, 0.125, 0, None)),
        'null/segnb_head_fwd': ('segnb_head_fwd', (nv.BF16, None, ld, N, H, W, C, X, X, 3, X, None)),
        'null/segnb_head_bwd': ('segnb_head_bwd', (nv.BF16, X, ld, *geoc, None, 3, X, X, ld, X, X, None)),
        'null/segnb_head_conv_fwd': ('segnb_head_conv_fwd', (nv.BF16, X, ld, N, H, W, C, None, 2, 2, 1, X, 1, X, None)),
        'null/segnb_head_conv_bwd': head_conv_bwd(a=None),
        # ---- the checks the issue names
        'no_gradient_source/reduce': reduce(gd=None),
        'no_gradient_source/apply_fused_src': fused_apply('segnb_bn_bwd_apply_fused_src',
                                                          tail=(1, SLOPE, None, None, 0, None, 0, None, 0, X + 64, ld)),
        'no_dz_no_sums/reduce': reduce(dz=None, sums=None),
        'no_dz_no_sums/reduce_add': ('segnb_bn_act_bwd_reduce_add',
                                     (nv.BF16, X, ld, *geo, X, 1, SLOPE, None, X, ld, X, ld, None, 0, None, None, 0, None)),
        'residual_and_pooled/reduce': reduce(gp=X, res=X),
        'residual_and_pooled/with_bad_dtype': reduce(BAD, gp=X, res=X),
        'dy_aliases_source/apply_fused_src': fused_apply('segnb_bn_bwd_apply_fused_src',
                                                         tail=(1, SLOPE, None, X, ld, None, 0, None, 0, X, ld)),
        'fused_head/k5': ('segnb_bn_fwd_fused_head', (nv.BF16, X, ld, *geoc, X, *bnp, X, ld, X, X, 5, X, None)),
        'fused_head/k5_head_bn_bwd': ('segnb_head_bn_bwd', (nv.BF16, X, ld, *geoc, X, 1, SLOPE, None, X, 5, X, X, ld, X, X, X, None)),
        'fused_head/k5_head_bn_bwd_apply': fused_apply('segnb_head_bn_bwd_apply', tail=(1, SLOPE, None, X, 5, X, X, ld)),
        'fused_head/bad_strides': fused_apply('segnb_head_bn_bwd_apply', tail=(1, SLOPE, None, X, 3, X, X, 24)),
        'fused_head/chunks_not_a_power_of_two': ('segnb_bn_fwd_fused_head',
                                                 (nv.BF16, X, ld, N, H, W, 24, 24, X, *bnp, X, ld, X, X, 3, X, None)),
        'stats_ld/fused_ld': ('segnb_bn_fwd_fused_ld', (nv.BF16, X, ld, *geoc, X, Cp - 8, *bnp, X, ld, None)),
        'stats_ld/fwd_stats': ('segnb_bn_act_fwd_stats', (nv.BF16, X, ld, *geo, X, 1, SLOPE, None, X, ld, X, Cp - 8, None)),
        'stats_ld/bn_stats_ld': ('segnb_bn_stats_ld', (nv.BF16, X, ld, *geo, X, Cp - 8, None)),
        'own_buffer/fused_acc': fused_apply('segnb_bn_bwd_apply_fused_acc', tail=(X, ld, X, ld)),
        'own_buffer/fused_acc_and_missing_sums': fused_apply('segnb_bn_bwd_apply_fused_acc', sums=None, tail=(X, ld, X, ld)),
        'own_buffer/fused_direct_acc': fused_apply('segnb_bn_bwd_apply_fused_direct_acc', tail=(1, SLOPE, X, ld, X, ld)),
        'maxpool_bwd_add/no_index': ('segnb_maxpool_bwd_add', (nv.BF16, X, ld, X, ld, X, ld, N, H, W, Cp, 3, 2, 1, X, ld, None, None)),
        'maxpool/bad_window': ('segnb_maxpool_fwd', (nv.BF16, X, ld, *geo, 3, 2, 3, X, ld, None, None)),
        'maxpool/empty_output': ('segnb_maxpool_fwd', (nv.BF16, X, ld, N, 2, 2, Cp, 5, 1, 0, X, ld, None, None)),
        'head/k0': ('segnb_head_fwd', (nv.BF16, X, ld, N, H, W, C, X, X, 0, X, None)),
        'head/k33': ('segnb_head_fwd', (nv.BF16, X, ld, N, H, W, C, X, X, 33, X, None)),
        'head/k33_bwd': ('segnb_head_bwd', (nv.BF16, X, ld, *geoc, X, 33, X, X, ld, X, X, None)),
        'head/bad_shape': ('segnb_head_fwd', (nv.BF16, X, 24, N, H, W, C, X, X, 3, X, None)),
        'head/smem_wide': ('segnb_head_fwd', (nv.BF16, X, 512, N, H, W, 512, X, X, 32, X, None)),
        'head/smem_wide_with_bad_dtype': ('segnb_head_fwd', (BAD, X, 512, N, H, W, 512, X, X, 32, X, None)),
        'head_conv/not_ok_fwd': ('segnb_head_conv_fwd', (nv.BF16, X, ld, N, H, W, C, X, 3, 3, 1, X, 1, X, None)),
        'head_conv/not_ok_bwd': head_conv_bwd(K=3),
        'head_conv/cp_above_64': head_conv_bwd(Cp_=72, C_=64),
        'head_conv/cp_above_64_with_bad_dtype': head_conv_bwd(BAD, Cp_=72, C_=64),
        'head_conv/empty_output': ('segnb_head_conv_fwd', (nv.BF16, X, ld, N, 1, 1, C, X, 2, 2, 0, X, 1, X, None)),
    }
    return calls


# refusals that make a HIP call before they return (segnb_head_bn_bwd asks for its scratch buffer before it looks at the dtype):
# recorded and compared on the GPU only
def _gpu_refusal_calls():
    X, N, H, W, C, Cp, ld = 0x1000, 2, 8, 8, 30, 32, 40
    return {'dtype/segnb_head_bn_bwd': ('segnb_head_bn_bwd',
                                        (7, X, ld, N, H, W, C, Cp, X, 1, SLOPE, None, X, 3, X, X, ld, X, X, X, None))}


def _refuse(calls):
    lib = nv.load()
    out = {}
    for name in sorted(calls):
        fn, args = calls[name]
        rc = getattr(lib, fn)(*args)
        out[name] = [fn, rc, (lib.segnb_last_error() or b'').decode()]
    return out


def refusals():
    """{name: [entry point, status, message]}; needs the library, not a GPU"""
    return _refuse(_refusal_calls())


def gpu_refusals():
    return _refuse(_gpu_refusal_calls())


def row_dtypes(row):
    return ('f32',) if row.startswith(F32_ONLY) else DTYPES


def table_row(row, ran):
    """what the table keeps of a row: the entry points called, the outputs digested and those left out, and per dtype ONE
    SHA-256 over the lines 'output:SHA-256 of its buffer' in output order -- every output of every case is in it, and the table
    stays a few hundred lines.  ran: {case: run_case(case)}"""
    cases = [ran['%s:%s' % (row, dt)] for dt in row_dtypes(row)]
    assert all(c['entries'] == cases[0]['entries'] and sorted(c['sha']) == sorted(cases[0]['sha']) for c in cases), row
    return {'entries': cases[0]['entries'], 'outputs': sorted(cases[0]['sha']), 'excluded': cases[0]['excluded'],
            'sha': {dt: hashlib.sha256(''.join('%s:%s\n' % kv for kv in sorted(c['sha'].items())).encode()).hexdigest()
                    for dt, c in zip(row_dtypes(row), cases)}}


def record():
    ran = {c: run_case(c) for c in CASES}
    return {'rows': {row: table_row(row, ran) for row in ROWS}, 'refusals': refusals(), 'gpu_refusals': gpu_refusals()}


if __name__ == '__main__':
    a, b = record(), record()
    for row in ROWS:
        assert a['rows'][row] == b['rows'][row], ('not reproducible', row, a['rows'][row], b['rows'][row])
    assert a['refusals'] == b['refusals'] and a['gpu_refusals'] == b['gpu_refusals']
    for k, v in sorted(list(a['refusals'].items()) + list(a['gpu_refusals'].items())):
        print(k, v)
        assert v[1] == -1 and v[2], ('not refused by an argument check', k, v)
    print(len(CASES), 'cases,', sum(len(r['outputs']) * len(r['sha']) for r in a['rows'].values()), 'outputs')
    with open(sys.argv[1] if len(sys.argv) > 1 else JSON_PATH, 'w') as f:           # one line per row / refusal
        parts = ['"%s":{\n%s\n}' % (sec, ',\n'.join('%s:%s' % (json.dumps(k), json.dumps(v, sort_keys=True, separators=(',', ':')))
                                                   for k, v in sorted(a[sec].items()))) for sec in sorted(a)]
        f.write('{\n' + ',\n'.join(parts) + '\n}\n')
