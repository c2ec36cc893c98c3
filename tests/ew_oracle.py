"""A float64 oracle with the call surface of the element-wise C ABI (helper module: no fixtures, no pytest settings).

`Oracle` is a backend for segnb._native.set_backend_for_testing with one method per entry point that ew_table.ROWS calls.  It
runs on CPU tensors, reads its operands through the pointers it is handed, and is written from the mathematics of each
operation and the contract in include/segnb_hip.h (cited below as H:<line>) -- not from a kernel and not from
oracle/abi_emulator.py:

  BatchNorm forward / backward   the four phases of inplace-ABN (H:251-252): mean_var, forward z = (y - mean) * scale + beta
                                 (H:256), edz_eydz (sum dz, sum dz * yhat, H:277) and dy = a * (dz - c1 - yhat * c2) (H:364)
  MaxPool                        nn.MaxPool2d, floor mode, gradient to the FIRST maximum of a window in row-major order (H:393-394)
  bilinear x 2                   align_corners=False (H:395): source coordinate (dst + 0.5) / 2 - 0.5 clamped at 0, the backward
                                 is the transpose
  classifier                     logits = bias + sum a * w (H:621), da / dw / db of H:613, H:625-626
  SGD / RMSprop / Adam           as torch defines them (H:743-748)

Arithmetic.  Everything is float64.  The only roundings applied are the ones the ABI specifies:

  R1  an output is rounded once to its storage type (bf16 round to nearest even, or fp32)                      H:17
  R2  dz is rounded to the storage type before it is summed ("Writes dz; accumulates ... sum dz")              H:276-278, H:436
  R3  pooling compares the activations as stored: pool_out = MaxPool2d(2) of a, routing to the first maximum   H:269, H:330
  R4  reduce_add: g = round(g_direct + g_add), "exactly what segnb_add would have stored"                      H:285
  R5  apply_direct / fused_direct / fused_src: dz "rounded to the storage type exactly as
      segnb_bn_act_bwd_reduce would have stored it"                                                           H:370-371, H:329-330
  R6  fused_acc / fused_direct_acc: "the result, rounded to the storage type, is added to the stored value"    H:314-315
  R7  maxpool_bwd_add routes round(g_out + g_out2)                                                             H:411
  R8  fused_head: the head reads the activated values rounded to the storage type                              H:666-667
  R9  head_bn_bwd(_apply): da "rounded to the storage type as it would have been stored"                       H:668, H:682
  R10 head_conv_bwd with an activation: dz = round(round(g) * act'(a))                                         H:628
  R11 pack_input_u8: v = (u8 * scale - mean) * (1 / std) "in fp32": the reciprocal is rounded to fp32          H:211
  R12 coef, bcoef, the running statistics, dgamma / dbeta and the optimizer state are fp32 (H:256, H:353): one
      fp32 rounding of the float64 value, one more for scale = gamma * invstd

What a value carries.  `X` holds the float64 value `v` and `e`, a per-element bound on |fp32 chain - v| BEFORE the store.
e == 0 means exact: every intermediate of the element, as a kernel working in fp32 holds it, is an fp32 number, so whatever
the order, the FMA contraction or the block arrival order, the stored result is the float64 result rounded once.  It is
checked on the float64 values, operation by operation (`_op`: operands exact and the result round-trips through fp32); for a
sum of n terms (`fsum`) the condition is  sum |x_i| <= 2^24 * g,  g the largest power of two that divides every term: every
partial sum is then a multiple of g below 2^24 g, an fp32 number.

The bound (where e > 0), derived as errbound.py derives its own.  An fp32 operation returns (a op b)(1 + d), |d| <= U_ACC,
so with operand errors ea, eb:
    add / sub      e = ea + eb + U_ACC * (|v| + ea + eb)
    mul            e = |a| eb + |b| ea + ea eb + U_ACC * (|v| + that)
    sum of n       e = sum e_i + n * U_ACC * sum |x_i|                      (any order; errbound's gamma_K * mag)
    act, max       Lipschitz 1 (slope: one more mul): e passes through
which is "number of fp32 operations * U_ACC * the operands' magnitudes" evaluated along the chain.  The first operation on two
stored operands, y - mean, is charged U_ACC * |y - mean|, not U_ACC * (|y| + |mean|): an fp32 subtraction is relatively exact
in its RESULT.  That is what makes the bound fail a cancelling formulation z = y * scale + (beta - mean * scale), whose error
is U_ACC * |y * scale|.  The operation counts per family are tabulated in DESIGN.md ("Element-wise passes against a float64
oracle").  At the store,
    bound = errbound.bound_of(v, e / U_ACC, 1, dtype) = r_out |v| (1 + 2^-8) + e (1 + r_out) + 2^-126
with r_out = R_BF16 for bf16 and 0 for fp32.  The casts of R12 are one `_op` each: e = U_ACC * |v| unless v is an fp32 number.

Discontinuities.  act' at z = 0 and the pool's argmax.  An element is ambiguous when |z| <= e_z with e_z > 0, or when the
first maximum of its window and another activation can change order: a kernel stores round(v') with |v' - v| <= e, rounding is
monotonic, so its value lies in [round(v - e), round(v + e)], and the order is open where two such intervals meet.
Exact values are never ambiguous: the tie rule decides (act'(0) is the negative side, the first maximum wins).  An element
whose gradient is zero on either side is not ambiguous.  Ambiguous elements are left out of the comparison (at most MAX_LEFT_OUT
of an output: asserted by the tests, checked on the CPU with the oracle alone) and 2 |g| is added to their e, so every sum over
them carries their magnitude in its bound.

Replicated tables ([16][2][ld]: stats, sums, out_stats) are compared as their sum over the replicas; the oracle adds into
replica 0.  Everything outside the region an entry point is specified to write -- padding columns, sentinels -- is compared
bit for bit with the buffer the oracle run leaves.
"""
import ctypes
import os

import numpy as np
import torch
import torch.nn.functional as F

import errbound as eb

U, R_BF16, TINY = eb.U_ACC, eb.R_BF16, eb.TINY
REPL = 16
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
MAX_LEFT_OUT = 0.01
TD = {'bf16': torch.bfloat16, 'f32': torch.float32, 'f64': torch.float64, 'u8': torch.uint8, 'i64': torch.int64,
      'i32': torch.int32}
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'ew_oracle_ratios.txt')


def _name(code):
    return 'bf16' if code == 1 else 'f32'


def _mem(ptr, numel, dtype):
    if isinstance(ptr, ctypes.c_void_p):
        ptr = ptr.value
    nbytes = numel * torch.empty((), dtype=dtype).element_size()
    return torch.frombuffer((ctypes.c_char * nbytes).from_address(int(ptr)), dtype=dtype)


def _view(ptr, shape, strides, dtype):
    n = 1 + sum((s - 1) * st for s, st in zip(shape, strides))
    return torch.as_strided(_mem(ptr, n, dtype), tuple(shape), tuple(strides))


def _f32(x):
    """a C float argument as the float64 number the library receives"""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ values with an error bound
class X(object):
    __slots__ = ('v', 'e')

    def __init__(self, v, e=None):
        self.v = v.double() if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float64)
        self.e = torch.zeros_like(self.v) if e is None else e

    def __getitem__(self, i):
        return X(self.v[i], self.e[i])

    def map(self, fn):
        return X(fn(self.v), fn(self.e))

    @property
    def exact(self):
        return not bool((self.e != 0).any())


def _fl(v):
    return v.float().double()


def _op(v, prop, clean_in=True):
    """the result of one fp32 operation whose exact value is v and whose operands' errors propagate to prop"""
    prop = torch.broadcast_to(torch.as_tensor(prop, dtype=torch.float64), v.shape)
    clean = (prop == 0) & (_fl(v) == v) & clean_in
    return X(v, torch.where(clean, torch.zeros_like(v), prop + U * (v.abs() + prop)))


def add(a, b):
    return _op(a.v + b.v, a.e + b.e)


def sub(a, b):
    return _op(a.v - b.v, a.e + b.e)


def mul(a, b):
    return _op(a.v * b.v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e)


def div(a, b):
    q = a.v / b.v
    return _op(q, (a.e + q.abs() * b.e) / (b.v.abs() - b.e).clamp(min=TINY))


def sqrt(a):
    s = a.v.sqrt()
    return _op(s, torch.where(a.e == 0, a.e, a.e / (a.v - a.e).clamp(min=TINY).sqrt()))


def cast(v):
    """R12: a float64 value stored as fp32"""
    return _op(v, 0.0)


def granularity(v):
    """the largest power of two that divides every element (1 for an all-zero tensor)"""
    nz = v[v != 0]
    if nz.numel() == 0:
        return 1.0
    m, ex = torch.frexp(nz)
    mi = (m.abs() * 2.0 ** 53).long()
    low = (mi & -mi).double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), (ex - 53).double())
    return float(low.min())


def fsum(x, dim):
    """n terms added in fp32 in any order"""
    n = x.v.shape[dim]
    v, mag, prop = x.v.sum(dim), x.v.abs().sum(dim), x.e.sum(dim)
    clean = (prop == 0) & (mag <= 2.0 ** 24 * granularity(x.v))
    return X(v, torch.where(clean, torch.zeros_like(v), prop + n * U * mag))


def stack(xs, dim=0):
    shape = torch.broadcast_shapes(*[x.v.shape for x in xs])
    return X(torch.stack([x.v.expand(shape) for x in xs], dim), torch.stack([x.e.expand(shape) for x in xs], dim))


def rnd(v, dt):
    """R1: the float64 value rounded once to the storage type"""
    return eb.round_out(v, dt).double() if dt in ('bf16', 'f32') else v.double()


def bound(x, dt):
    b = eb.bound_of(x.v, x.e / U, 1, dt)
    return torch.where(x.e == 0, torch.zeros_like(b), b)


def stored(x, dt):
    """what the next reader finds: the rounded value, and how far a kernel's own stored value may be from it"""
    return X(rnd(x.v, dt), bound(x, dt))


class Note(object):
    """what the oracle says about one output: region (shape, strides in elements from the buffer's start), float64 value,
    per-element bound (0: compared with ==), the elements left out, whether it is a replicated table"""
    def __init__(self, shape, strides, ref, err, amb, dt, repl):
        self.shape, self.strides, self.ref, self.err, self.amb, self.dt, self.repl = shape, strides, ref, err, amb, dt, repl

    @property
    def exact(self):
        return not bool((self.err != 0).any())


# ------------------------------------------------------------------------------------------------ the backend
class Oracle(object):
    def __init__(self):
        self.notes = {}

    # ---- plumbing
    def put(self, ptr, shape, strides, x, dt, amb=None, is_stored=False, repl=False):
        shape = tuple(shape)
        x = X(x.v.expand(shape[1:] if repl else shape).clone(), x.e.expand(shape[1:] if repl else shape).clone())
        err = x.e if (is_stored or repl) else bound(x, dt)
        if amb is not None:
            amb = amb.expand(shape).clone()
            assert not bool((amb & (err == 0)).any()), 'an exact element cannot be ambiguous'
        if not repl:
            _view(ptr, shape, strides, TD[dt]).copy_(rnd(x.v, dt).to(TD[dt]))
        self.notes[int(ptr)] = Note(shape, tuple(strides), x.v, err, amb, dt, repl)
        return X(rnd(x.v, dt), err.clone())

    def pix(self, ptr, N, H, W, C, ld, dt):
        return X(_view(ptr, (N, H, W, C), (H * W * ld, W * ld, ld, 1), TD[dt]))

    def put_pix(self, ptr, N, H, W, C, ld, x, dt, amb=None, is_stored=False):
        return self.put(ptr, (N, H, W, C), (H * W * ld, W * ld, ld, 1), x, dt, amb, is_stored)

    def vec(self, ptr, n, default=None):
        if ptr is None:
            return X(torch.full((n,), float(default), dtype=torch.float64))
        return X(_mem(ptr, n, torch.float32).clone())

    def table(self, ptr, Cp, ld=None):
        ld = ld or Cp
        return _view(ptr, (REPL, 2, Cp), (2 * ld, ld, 1), torch.float64)

    def accumulate_table(self, ptr, Cp, ld, s):
        """s: X [2][Cp] added to a replicated table"""
        t = self.table(ptr, Cp, ld)
        total = X(t.sum(0) + s.v, s.e)
        t[0] += s.v
        self.put(ptr, (REPL, 2, Cp), (2 * (ld or Cp), ld or Cp, 1), total, 'f64', repl=True)

    def clear_table(self, ptr, Cp):
        if ptr is not None:
            self.put(ptr, (REPL, 2, Cp), (2 * Cp, Cp, 1), X(torch.zeros(REPL, 2, Cp)), 'f64')

    def chan_sum(self, x):
        """[pixels][C] -> per-channel sum"""
        return fsum(x, 0)

    # ---- BatchNorm forward
    def coefs(self, coef, Cp):
        if coef is None:
            return None
        c = X(_mem(coef, 4 * Cp, torch.float32).view(4, Cp).clone())
        return c[0], c[1], c[2], c[3]               # scale, beta, mean, invstd (H:256)

    def z_of(self, Y, co, res):
        z = Y
        if co is not None:
            scale, beta, mean, _ = co
            z = add(mul(sub(Y, mean), scale), beta)
        return z if res is None else add(z, res)

    def act_of(self, z, act, slope):
        """-> activated value, act'(z), ambiguous elements"""
        amb = (z.v.abs() <= z.e) & (z.e > 0)
        if act == ACT_NONE:
            return z, None, torch.zeros_like(amb)
        pos = z.v > 0
        sl = _f32(slope) if act == ACT_LEAKY else 0.0
        neg = mul(z, X(sl)) if act == ACT_LEAKY else X(torch.zeros_like(z.v))       # (ReLU of a clearly negative z is exactly 0)
        e = torch.where(amb, torch.maximum(z.e, neg.e), torch.where(pos, z.e, neg.e))
        grad = torch.where(pos, torch.ones_like(z.v), torch.full_like(z.v, sl))
        return X(torch.where(pos, z.v, neg.v), e), X(grad), amb

    def drop_table(self, dropmul, N, Cp):
        if dropmul is None:
            return None
        return X(_mem(dropmul, N * Cp, torch.float32).view(N, 1, 1, Cp).clone())

    def activated(self, Y, co, act, slope, dm, res):
        z = self.z_of(Y, co, res)
        a, grad, amb = self.act_of(z, act, slope)
        return z, (a if dm is None else mul(a, dm)), grad, amb

    @staticmethod
    def windows(t, Hp, Wp):
        """[N,H,W,C] -> [N,Hp,Wp,4,C], window positions in row-major order"""
        N, C = t.shape[0], t.shape[3]
        return t[:, :2 * Hp, :2 * Wp].reshape(N, Hp, 2, Wp, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, Hp, Wp, 4, C)

    @staticmethod
    def unwindows(w, H, W):
        N, Hp, Wp, _, C = w.shape
        out = torch.zeros(N, H, W, C, dtype=w.dtype)
        out[:, :2 * Hp, :2 * Wp] = w.reshape(N, Hp, Wp, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * Hp, 2 * Wp, C)
        return out

    def pooled(self, A, H, W):
        """MaxPool2d(2), floor mode, of the stored activations (H:269): an odd last row or column is in no window"""
        return X(self.windows(A.v, H // 2, W // 2).amax(3), self.windows(A.e, H // 2, W // 2).amax(3))

    def forward_outputs(self, dt, a, N, H, W, Cp, out, ld_out, pool_out, ld_pool, up_out, ld_up):
        A = stored(a, dt)
        if out is not None:
            self.put_pix(out, N, H, W, Cp, ld_out, a, dt)
        if pool_out is not None:
            self.put_pix(pool_out, N, H // 2, W // 2, Cp, ld_pool, self.pooled(A, H, W), dt, is_stored=True)
        if up_out is not None:
            self.put_pix(up_out, N, 2 * H, 2 * W, Cp, ld_up,
                         A.map(lambda t: t.repeat_interleave(2, 1).repeat_interleave(2, 2)), dt, is_stored=True)
        return A

    def segnb_bn_act_fwd(self, dtype, y, ld_y, N, H, W, Cp, coef, act, slope, dropmul, out, ld_out, pool_out, ld_pool, up_out,
                         ld_up, res, ld_res, stream, _co=None):
        dt = _name(dtype)
        Y = self.pix(y, N, H, W, Cp, ld_y, dt)
        Rs = self.pix(res, N, H, W, Cp, ld_res, dt) if res is not None else None
        co = _co or self.coefs(coef, Cp)
        _, a, _, _ = self.activated(Y, co, act, slope, self.drop_table(dropmul, N, Cp), Rs)
        return self.forward_outputs(dt, a, N, H, W, Cp, out, ld_out, pool_out, ld_pool, up_out, ld_up) and 0

    def stats_of(self, A):
        """[N,H,W,C] stored values -> X [2][C]: sum, sum of squares (H:389)"""
        flat = A.map(lambda t: t.reshape(-1, t.shape[-1]))
        return stack([self.chan_sum(flat), self.chan_sum(mul(flat, flat))])

    def segnb_bn_stats(self, dtype, x, ld, N, H, W, Cp, stats, stream):
        return self.segnb_bn_stats_ld(dtype, x, ld, N, H, W, Cp, stats, Cp, stream)

    def segnb_bn_stats_ld(self, dtype, x, ld, N, H, W, Cp, stats, stats_ld, stream):
        self.accumulate_table(stats, Cp, stats_ld, self.stats_of(self.pix(x, N, H, W, Cp, ld, _name(dtype))))
        return 0

    def segnb_bn_act_fwd_stats(self, dtype, y, ld_y, N, H, W, Cp, coef, act, slope, dropmul, out, ld_out, out_stats, out_stats_ld,
                               stream):
        dt = _name(dtype)
        Y = self.pix(y, N, H, W, Cp, ld_y, dt)
        _, a, _, _ = self.activated(Y, self.coefs(coef, Cp), act, slope, self.drop_table(dropmul, N, Cp), None)
        A = self.forward_outputs(dt, a, N, H, W, Cp, out, ld_out, None, 0, None, 0)
        self.accumulate_table(out_stats, Cp, out_stats_ld, self.stats_of(A))
        return 0

    # ---- the finalizes
    def finalize(self, S, C, Cp, count, gamma, beta, eps, momentum, rm, rv, nbt, training, coef):
        """S: float64 [2][Cp] sums over the replicas.  -> (scale, beta, mean, invstd) as the activation pass reads them"""
        count, eps, m = float(count), _f32(eps), _f32(momentum)
        if training:
            mu = S[0, :C] / count
            var = (S[1, :C] / count - mu * mu).clamp(min=0)         # biased, as nn.BatchNorm2d normalises
            if rm is not None:
                unb = var * count / (count - 1.0) if count > 1 else var
                self.put(rm, (C,), (1,), cast((1 - m) * _mem(rm, C, torch.float32).double() + m * mu), 'f32')
                self.put(rv, (C,), (1,), cast((1 - m) * _mem(rv, C, torch.float32).double() + m * unb), 'f32')
            if nbt is not None:
                self.put(nbt, (1,), (1,), X(_mem(nbt, 1, torch.int64).double() + 1), 'i64')
        else:
            mu, var = _mem(rm, C, torch.float32).double(), _mem(rv, C, torch.float32).double()
        invstd = cast(1.0 / torch.sqrt(var + eps))
        rows = [mul(self.vec(gamma, C, 1.0), stored(invstd, 'f32')), self.vec(beta, C, 0.0), cast(mu), invstd]
        pad = lambda t: torch.cat([t, torch.zeros(Cp - C, dtype=torch.float64)])
        co = self.put(coef, (4, Cp), (Cp, 1), stack([r.map(pad) for r in rows]), 'f32')
        return co[0], co[1], co[2], co[3]

    def segnb_bn_finalize(self, stats, C, Cp, count, gamma, beta, eps, momentum, rm, rv, nbt, training, coef, stream):
        S = self.table(stats, Cp).sum(0) if training else None
        self.finalize(S, C, Cp, count, gamma, beta, eps, momentum, rm, rv, nbt, training, coef)
        if training:
            self.clear_table(stats, Cp)                             # CONSUMED (H:258)
        return 0

    def segnb_bn_finalize_keep(self, stats, C, Cp, count, gamma, beta, eps, momentum, rm, rv, nbt, coef, clear_sums, stream):
        self.finalize(self.table(stats, Cp).sum(0), C, Cp, count, gamma, beta, eps, momentum, rm, rv, nbt, 1, coef)
        self.clear_table(clear_sums, Cp)
        return 0

    def segnb_bn_fwd_fused_ld(self, dtype, y, ld_y, N, H, W, C, Cp, stats, stats_ld, gamma, beta, eps, momentum, rm, rv, nbt, coef,
                              clear_sums, act, slope, dropmul, out, ld_out, stream, _rest=(None, 0, None, 0, None, 0)):
        co = self.finalize(self.table(stats, Cp, stats_ld).sum(0), C, Cp, N * H * W, gamma, beta, eps, momentum, rm, rv, nbt, 1, coef)
        self.clear_table(clear_sums, Cp)
        return self.segnb_bn_act_fwd(dtype, y, ld_y, N, H, W, Cp, None, act, slope, dropmul, out, ld_out, *_rest, stream, _co=co)

    def segnb_bn_fwd_fused(self, dtype, y, ld_y, N, H, W, C, Cp, stats, gamma, beta, eps, momentum, rm, rv, nbt, coef, clear_sums,
                           act, slope, dropmul, out, ld_out, pool_out, ld_pool, up_out, ld_up, res, ld_res, stream):
        return self.segnb_bn_fwd_fused_ld(dtype, y, ld_y, N, H, W, C, Cp, stats, Cp, gamma, beta, eps, momentum, rm, rv, nbt, coef,
                                          clear_sums, act, slope, dropmul, out, ld_out, stream,
                                          _rest=(pool_out, ld_pool, up_out, ld_up, res, ld_res))

    def segnb_head_fused_ok(self, K, Cp):
        q = Cp // 8
        return int(1 <= K <= 4 and Cp % 8 == 0 and 8 <= Cp <= 256 and q & (q - 1) == 0)     # H:671

    def segnb_bn_fwd_fused_head(self, dtype, y, ld_y, N, H, W, C, Cp, stats, gamma, beta, eps, momentum, rm, rv, nbt, coef,
                                clear_sums, act, slope, dropmul, out, ld_out, head_w, head_b, K, logits, stream):
        dt = _name(dtype)
        co = self.finalize(self.table(stats, Cp).sum(0), C, Cp, N * H * W, gamma, beta, eps, momentum, rm, rv, nbt, 1, coef)
        self.clear_table(clear_sums, Cp)
        Y = self.pix(y, N, H, W, Cp, ld_y, dt)
        _, a, _, _ = self.activated(Y, co, act, slope, self.drop_table(dropmul, N, Cp), None)
        A = self.forward_outputs(dt, a, N, H, W, Cp, out, ld_out, None, 0, None, 0)        # R8
        self.head_logits(A[..., :C], head_w, head_b, K, logits)
        return 0

    # ---- BatchNorm backward: reduction
    @staticmethod
    def first_of(is_max, dim):
        """the first maximum in window order (H:394)"""
        return is_max & (is_max.cumsum(dim) == 1)

    @staticmethod
    def up_taps():
        """the 2 x 2 high-resolution pixels behind one pixel of a nearest x 2 upsample"""
        return [(0, 0), (0, 1), (1, 0), (1, 1)]

    def gradient(self, dt, a, N, H, W, Cp, g_direct, ld_gd, g_pool, ld_gp, g_up, ld_gu):
        """g_direct + maxpool_bwd(g_pool) + upsample_bwd(g_up) (H:276) -> X, ambiguous elements"""
        terms, amb = [], torch.zeros(N, H, W, Cp, dtype=torch.bool)
        if g_direct is not None:
            terms.append(self.pix(g_direct, N, H, W, Cp, ld_gd, dt))
        if g_pool is not None:
            Hp, Wp = H // 2, W // 2
            gp = self.pix(g_pool, N, Hp, Wp, Cp, ld_gp, dt).v
            # R3: the activations as stored.  A kernel stores round(v') with |v' - v| <= e, and rounding is monotonic: its value
            # lies in [lo, hi]; two elements can change order only where those intervals meet
            wv = self.windows(rnd(a.v, dt), Hp, Wp)
            lo, hi = self.windows(rnd(a.v - a.e, dt), Hp, Wp), self.windows(rnd(a.v + a.e, dt), Hp, Wp)
            is_max = wv == wv.amax(3, keepdim=True)
            first = self.first_of(is_max, 3)
            top_lo, top_sure = (lo * first).sum(3, keepdim=True), ((lo == hi) & first).any(3, keepdim=True)
            close = ((~first) & (hi >= top_lo) & ~((lo == hi) & top_sure)).any(3, keepdim=True) & (gp[:, :, :, None, :] != 0)
            amb_w = close.expand_as(wv).double()                    # the whole window: its gradient may land on any of them
            terms.append(X(self.unwindows(first.double() * gp[:, :, :, None, :], H, W),
                           self.unwindows(amb_w * gp[:, :, :, None, :].abs(), H, W)))
            amb |= self.unwindows(amb_w, H, W) > 0
        if g_up is not None:
            gu = self.pix(g_up, N, 2 * H, 2 * W, Cp, ld_gu, dt)
            terms += [gu.map(lambda t: t[:, i::2, j::2]) for i, j in self.up_taps()]
        return fsum(stack(terms), 0), amb

    def dz_of(self, dt, y, ld_y, N, H, W, Cp, co, act, slope, dropmul, sources, res, ld_res, g=None):
        """-> Y, dz as stored (R2), ambiguous elements"""
        Y = self.pix(y, N, H, W, Cp, ld_y, dt)
        Rs = self.pix(res, N, H, W, Cp, ld_res, dt) if res is not None else None
        dm = self.drop_table(dropmul, N, Cp)
        z, a, grad, amb = self.activated(Y, co, act, slope, dm, Rs)
        if g is None:
            g, amb_pool = self.gradient(dt, a, N, H, W, Cp, *sources)
            amb = amb | amb_pool
        gm = g if dm is None else mul(g, dm)
        d = gm if grad is None else mul(gm, grad)
        amb = amb & ((gm.v != 0) | (gm.e != 0))                     # (a zero gradient stays zero on either side)
        d = X(d.v, d.e + 2 * (gm.v.abs() + gm.e) * amb)             # act' is 0 .. 1: either side is within that
        return Y, d, amb

    @staticmethod
    def summed_dz(d, D, dt):
        """what the sums are taken over: dz as stored (R2), not the value before its rounding"""
        return D

    def reduce_sums(self, Y, dz, amb, co, Cp, sums):
        """sums[0] += sum dz, sums[1] += sum dz * yhat over the STORED dz (R2); ambiguous elements carry their magnitude"""
        flat = lambda x: x.map(lambda t: t.expand(Y.v.shape).reshape(-1, Cp))
        rows = [self.chan_sum(flat(dz))]
        if co is not None:
            rows.append(mul(self.chan_sum(flat(mul(dz, sub(Y, co[2])))), co[3]))
        else:
            rows.append(X(torch.zeros(Cp)))
        self.accumulate_table(sums, Cp, Cp, stack(rows))

    def segnb_bn_act_bwd_reduce(self, dtype, y, ld_y, N, H, W, Cp, coef, act, slope, dropmul, g_direct, ld_gd, g_pool, ld_gp, g_up,
                                ld_gu, dz, ld_dz, sums, res, ld_res, stream, _g=None):
        dt = _name(dtype)
        co = self.coefs(coef, Cp)
        Y, d, amb = self.dz_of(dt, y, ld_y, N, H, W, Cp, co, act, slope, dropmul, (g_direct, ld_gd, g_pool, ld_gp, g_up, ld_gu),
                               res, ld_res, _g)
        D = self.put_pix(dz, N, H, W, Cp, ld_dz, d, dt, amb) if dz is not None else stored(d, dt)
        if sums is not None:
            self.reduce_sums(Y, self.summed_dz(d, D, dt), amb, co, Cp, sums)
        return 0

    def segnb_bn_act_bwd_reduce_add(self, dtype, y, ld_y, N, H, W, Cp, coef, act, slope, dropmul, g_direct, ld_gd, g_add, ld_ga,
                                    dz, ld_dz, sums, res, ld_res, stream):
        dt = _name(dtype)
        g = stored(add(self.pix(g_direct, N, H, W, Cp, ld_gd, dt), self.pix(g_add, N, H, W, Cp, ld_ga, dt)), dt)      # R4
        return self.segnb_bn_act_bwd_reduce(dtype, y, ld_y, N, H, W, Cp, coef, act, slope, dropmul, None, 0, None, 0, None, 0,
                                            dz, ld_dz, sums, res, ld_res, stream, _g=g)

    # ---- BatchNorm backward: finalize and apply
    def accumulated(self, ptr, C, new):
        """dgamma / dbeta += (H:353)"""
        return add(self.vec(ptr, C), new)

    def bwd_finalize(self, S, C, Cp, count, gamma, co, bcoef, dgamma, dbeta, accumulate):
        """S: float64 [2][Cp].  bcoef = (gamma * invstd, mean(dz), mean(dz * yhat)) (H:353); dgamma / dbeta assigned or
        accumulated -> the three rows as the apply pass reads them"""
        pad = lambda t: torch.cat([t, torch.zeros(Cp - C, dtype=torch.float64)])
        rows = [mul(self.vec(gamma, C, 1.0), co[3][:C]), cast(S[0, :C] / float(count)), cast(S[1, :C] / float(count))]
        bc = self.put(bcoef, (3, Cp), (Cp, 1), stack([r.map(pad) for r in rows]), 'f32')
        for ptr, row in ((dgamma, 1), (dbeta, 0)):
            if ptr is not None:
                new = stored(cast(S[row, :C]), 'f32')
                if accumulate:
                    new = self.accumulated(ptr, C, new)
                self.put(ptr, (C,), (1,), new, 'f32')
        return bc

    def segnb_bn_bwd_finalize_clear(self, sums, C, Cp, count, gamma, coef, bcoef, dgamma, dbeta, accumulate, clear, stream):
        self.bwd_finalize(self.table(sums, Cp).sum(0), C, Cp, count, gamma, self.coefs(coef, Cp), bcoef, dgamma, dbeta, accumulate)
        self.clear_table(sums, Cp)                                  # CONSUMED (H:354)
        self.clear_table(clear, Cp)
        return 0

    def segnb_bn_bwd_finalize(self, sums, C, Cp, count, gamma, coef, bcoef, dgamma, dbeta, accumulate, stream):
        return self.segnb_bn_bwd_finalize_clear(sums, C, Cp, count, gamma, coef, bcoef, dgamma, dbeta, accumulate, None, stream)

    @staticmethod
    def dy_of(Y, co, bc, dz):
        """dy = a * (dz - c1 - yhat * c2), yhat = (y - mean) * invstd (H:364)"""
        yhat = mul(sub(Y, co[2]), co[3])
        return mul(bc[0], sub(sub(dz, bc[1]), mul(yhat, bc[2])))

    def apply(self, dt, Y, co, bc, dz, amb, N, H, W, Cp, dy, ld_dy, dbias, C, acc=False):
        d = self.dy_of(Y, co, bc, dz)
        if acc:                                                     # R6
            d = add(self.pix(dy, N, H, W, Cp, ld_dy, dt), stored(d, dt))
        D = self.put_pix(dy, N, H, W, Cp, ld_dy, d, dt, amb)
        if dbias is not None:                                       # dbias[c] += sum dy, fp32 (H:365)
            s = self.chan_sum(D.map(lambda t: t.reshape(-1, Cp)))[:C]
            self.put(dbias, (C,), (1,), add(self.vec(dbias, C), s), 'f32')
        return 0

    def segnb_bn_bwd_apply(self, dtype, y, ld_y, N, H, W, Cp, coef, bcoef, dz, ld_dz, dy, ld_dy, dbias, C, stream):
        dt = _name(dtype)
        bc = X(_mem(bcoef, 3 * Cp, torch.float32).view(3, Cp).clone())
        return self.apply(dt, self.pix(y, N, H, W, Cp, ld_y, dt), self.coefs(coef, Cp), bc, self.pix(dz, N, H, W, Cp, ld_dz, dt),
                          None, N, H, W, Cp, dy, ld_dy, dbias, C)

    def segnb_bn_bwd_apply_direct(self, dtype, y, ld_y, N, H, W, Cp, coef, bcoef, act, slope, g, ld_g, dy, ld_dy, dbias, C, stream):
        dt = _name(dtype)
        co = self.coefs(coef, Cp)
        bc = X(_mem(bcoef, 3 * Cp, torch.float32).view(3, Cp).clone())
        Y, d, amb = self.dz_of(dt, y, ld_y, N, H, W, Cp, co, act, slope, None, (g, ld_g, None, 0, None, 0), None, 0)
        return self.apply(dt, Y, co, bc, stored(d, dt), amb, N, H, W, Cp, dy, ld_dy, dbias, C)          # R5

    def fused_apply(self, dtype, y, ld_y, N, H, W, C, Cp, coef, sums, gamma, bcoef, dgamma, dbeta, accumulate, clear_stats, dy,
                    ld_dy, dz=None, ld_dz=0, act=ACT_NONE, slope=0.0, dropmul=None, sources=None, g=None, acc=False):
        dt = _name(dtype)
        co = self.coefs(coef, Cp)
        bc = self.bwd_finalize(self.table(sums, Cp).sum(0), C, Cp, N * H * W, gamma, co, bcoef, dgamma, dbeta, accumulate)
        self.clear_table(clear_stats, Cp)                           # `sums` is NOT consumed here (H:307)
        if dz is not None:
            Y, D, amb = self.pix(y, N, H, W, Cp, ld_y, dt), self.pix(dz, N, H, W, Cp, ld_dz, dt), None
        else:
            Y, d, amb = self.dz_of(dt, y, ld_y, N, H, W, Cp, co, act, slope, dropmul, sources, None, 0, g)
            D = stored(d, dt)                                       # R5
        return self.apply(dt, Y, co, bc, D, amb, N, H, W, Cp, dy, ld_dy, None, C, acc)

    def segnb_bn_bwd_apply_fused(self, dtype, y, ld_y, N, H, W, C, Cp, coef, sums, gamma, bcoef, dgamma, dbeta, accumulate,
                                 clear_stats, dz, ld_dz, dy, ld_dy, stream, _acc=False):
        return self.fused_apply(dtype, y, ld_y, N, H, W, C, Cp, coef, sums, gamma, bcoef, dgamma, dbeta, accumulate, clear_stats,
                                dy, ld_dy, dz=dz, ld_dz=ld_dz, acc=_acc)

    def segnb_bn_bwd_apply_fused_acc(self, *a):
        return self.segnb_bn_bwd_apply_fused(*a, _acc=True)

    def segnb_bn_bwd_apply_fused_direct(self, dtype, y, ld_y, N, H, W, C, Cp, coef, sums, gamma, bcoef, dgamma, dbeta, accumulate,
                                        clear_stats, act, slope, g, ld_g, dy, ld_dy, stream, _acc=False):
        return self.fused_apply(dtype, y, ld_y, N, H, W, C, Cp, coef, sums, gamma, bcoef, dgamma, dbeta, accumulate, clear_stats,
                                dy, ld_dy, act=act, slope=slope, sources=(g, ld_g, None, 0, None, 0), acc=_acc)

    def segnb_bn_bwd_apply_fused_direct_acc(self, *a):
        return self.segnb_bn_bwd_apply_fused_direct(*a, _acc=True)

    def segnb_bn_bwd_apply_fused_src(self, dtype, y, ld_y, N, H, W, C, Cp, coef, sums, gamma, bcoef, dgamma, dbeta, accumulate,
                                     clear_stats, act, slope, dropmul, g_direct, ld_gd, g_pool, ld_gp, g_up, ld_gu, dy, ld_dy, stream):
        return self.fused_apply(dtype, y, ld_y, N, H, W, C, Cp, coef, sums, gamma, bcoef, dgamma, dbeta, accumulate, clear_stats,
                                dy, ld_dy, act=act, slope=slope, dropmul=dropmul,
                                sources=(g_direct, ld_gd, g_pool, ld_gp, g_up, ld_gu))

    def segnb_bias_grad_job_bytes(self):
        return 24

    def segnb_bias_grad_multi(self, jobs, njobs, stream):
        """gb += the sum over the replicas of row 0, then the sums are cleared (H:659)"""
        raw = bytes((ctypes.c_uint8 * (24 * njobs)).from_address(int(jobs)))
        for j in np.frombuffer(raw, dtype=np.dtype([('sums', '<u8'), ('gb', '<u8'), ('C', '<i4'), ('Cp', '<i4')])):
            C, Cp = int(j['C']), int(j['Cp'])
            if int(j['gb']):
                s = stored(cast(self.table(int(j['sums']), Cp).sum(0)[0, :C]), 'f32')
                self.put(int(j['gb']), (C,), (1,), add(self.vec(int(j['gb']), C), s), 'f32')
            self.clear_table(int(j['sums']), Cp)
        return 0

    def segnb_abn_scale(self, w, eps, out, n, stream):
        self.put(out, (n,), (1,), add(self.vec(w, n).map(torch.abs), X(_f32(eps))), 'f32')         # |w| + eps (H:340)
        return 0

    def segnb_abn_dscale(self, w, dscale, dw, n, stream):
        sign = X(torch.where(self.vec(w, n).v > 0, 1.0, -1.0))                                       # H:342
        self.put(dw, (n,), (1,), add(self.vec(dw, n), mul(sign, self.vec(dscale, n))), 'f32')
        self.put(dscale, (n,), (1,), X(torch.zeros(n)), 'f32')
        return 0

    # ---- classifier heads
    def head_logits(self, A, w, bias, K, logits):
        """logits[n][k][h][w] = bias[k] + sum_c a[n][h][w][c] * w[k][c], fp32 NCHW"""
        N, H, W, C = A.v.shape
        Wm = X(_mem(w, K * C, torch.float32).view(K, C).clone())
        terms = [mul(A.map(lambda t: t[..., None, :]), Wm)]
        if bias is not None:
            terms.append(self.vec(bias, K).map(lambda t: t.expand(N, H, W, K)[..., None]))
        out = fsum(X(torch.cat([t.v for t in terms], -1), torch.cat([t.e for t in terms], -1)), -1)
        self.put(logits, (N, K, H, W), (K * H * W, H * W, W, 1), out.map(lambda t: t.permute(0, 3, 1, 2)), 'f32')

    def segnb_head_fwd(self, dtype, a, ld_a, N, H, W, C, w, bias, K, logits, stream):
        self.head_logits(self.pix(a, N, H, W, C, ld_a, _name(dtype)), w, bias, K, logits)
        return 0

    def head_backward(self, dt, A, N, H, W, C, Cp, w, K, dlogits, dw, db):
        """-> da = dlogits . w over the Cp channels (zero beyond C) before its store; dw, db accumulated (H:613)"""
        Wm = X(_mem(w, K * C, torch.float32).view(K, C).clone())
        DL = X(_mem(dlogits, N * K * H * W, torch.float32).view(N, K, H, W).permute(0, 2, 3, 1).clone())
        da = fsum(mul(DL.map(lambda t: t[..., None]), Wm), 3)
        da = da.map(lambda t: F.pad(t, (0, Cp - C)))
        flat = DL.map(lambda t: t.reshape(-1, K))
        if dw is not None:
            s = self.chan_sum(mul(flat.map(lambda t: t[:, :, None]), A.map(lambda t: t.reshape(-1, 1, C))))
            self.put(dw, (K, C), (C, 1), add(self.vec(dw, K * C).map(lambda t: t.view(K, C)), s), 'f32')
        if db is not None:
            self.put(db, (K,), (1,), add(self.vec(db, K), self.chan_sum(flat)), 'f32')
        return da

    def segnb_head_bwd(self, dtype, a, ld_a, N, H, W, C, Cp, w, K, dlogits, da, ld_da, dw, db, stream):
        dt = _name(dtype)
        d = self.head_backward(dt, self.pix(a, N, H, W, C, ld_a, dt), N, H, W, C, Cp, w, K, dlogits, dw, db)
        self.put_pix(da, N, H, W, Cp, ld_da, d, dt)
        return 0

    def segnb_head_bn_bwd(self, dtype, y, ld_y, N, H, W, C, Cp, coef, act, slope, dropmul, head_w, K, dlogits, dz, ld_dz, sums, dw,
                          db, stream):
        dt = _name(dtype)
        Y = self.pix(y, N, H, W, Cp, ld_y, dt)
        _, a, _, _ = self.activated(Y, self.coefs(coef, Cp), act, slope, self.drop_table(dropmul, N, Cp), None)
        da = self.head_backward(dt, stored(a, dt)[..., :C], N, H, W, C, Cp, head_w, K, dlogits, dw, db)
        return self.segnb_bn_act_bwd_reduce(dtype, y, ld_y, N, H, W, Cp, coef, act, slope, dropmul, None, 0, None, 0, None, 0, dz,
                                            ld_dz, sums, None, 0, stream, _g=stored(da, dt))               # R9

    def segnb_head_bn_bwd_apply(self, dtype, y, ld_y, N, H, W, C, Cp, coef, sums, gamma, bcoef, dgamma, dbeta, accumulate,
                                clear_stats, act, slope, dropmul, head_w, K, dlogits, dy, ld_dy, stream):
        dt = _name(dtype)
        da = self.head_backward(dt, None, N, H, W, C, Cp, head_w, K, dlogits, None, None)
        return self.fused_apply(dtype, y, ld_y, N, H, W, C, Cp, coef, sums, gamma, bcoef, dgamma, dbeta, accumulate, clear_stats,
                                dy, ld_dy, act=act, slope=slope, dropmul=dropmul, g=stored(da, dt))

    def segnb_head_conv_ok(self, C, K, kh, kw):
        return int(K >= 1 and kh >= 1 and kw >= 1 and K * kh * kw <= 8 and 1 <= C <= 64)            # H:623

    @staticmethod
    def conv_x(fn, a, b, n_terms):
        """a bilinear map fn(a, b) of exact operands whose every element is a sum of at most n_terms products"""
        v, mag = fn(a, b), fn(a.abs(), b.abs())
        clean = mag <= 2.0 ** 24 * granularity(a) * granularity(b)
        return X(v, torch.where(clean, torch.zeros_like(v), n_terms * U * mag))

    def segnb_head_conv_fwd(self, dtype, a, ld_a, N, Hi, Wi, C, w, kh, kw, pad, bias, K, logits, stream):
        A = self.pix(a, N, Hi, Wi, C, ld_a, _name(dtype)).v.permute(0, 3, 1, 2)
        Wm = _mem(w, K * C * kh * kw, torch.float32).view(K, C, kh, kw).double()
        out = self.conv_x(lambda p, q: F.conv2d(p, q, padding=pad), A, Wm, C * kh * kw)
        if bias is not None:
            out = add(out, self.vec(bias, K).map(lambda t: t.view(1, K, 1, 1)))
        Ho, Wo = out.v.shape[2:]
        self.put(logits, (N, K, Ho, Wo), (K * Ho * Wo, Ho * Wo, Wo, 1), out, 'f32')
        return 0

    def segnb_head_conv_bwd(self, dtype, a, ld_a, N, Hi, Wi, C, Cp, w, kh, kw, pad, K, dlogits, act, slope, da, ld_da, dw, db, sums,
                            stream):
        dt = _name(dtype)
        Av = self.pix(a, N, Hi, Wi, Cp, ld_a, dt).v
        A = Av[..., :C].permute(0, 3, 1, 2)
        Wm = _mem(w, K * C * kh * kw, torch.float32).view(K, C, kh, kw).double()
        Ho, Wo = Hi + 2 * pad - kh + 1, Wi + 2 * pad - kw + 1
        DL = _mem(dlogits, N * K * Ho * Wo, torch.float32).view(N, K, Ho, Wo).double()
        g = self.conv_x(lambda p, q: F.conv_transpose2d(p, q, padding=pad), DL, Wm, K * kh * kw)       # H:626
        g = g.map(lambda t: F.pad(t.permute(0, 2, 3, 1), (0, Cp - C)))
        if act >= 0:                                                # R10: act' from the sign of the activated value
            neg = 0.0 if act == ACT_RELU else (_f32(slope) if act == ACT_LEAKY else 1.0)
            g = mul(stored(g, dt), X(torch.where(Av > 0, 1.0, neg)))
        D = self.put_pix(da, N, Hi, Wi, Cp, ld_da, g, dt)
        if act >= 0 and sums is not None:
            self.accumulate_table(sums, Cp, Cp, stack([self.chan_sum(D.map(lambda t: t.reshape(-1, Cp))), X(torch.zeros(Cp))]))
        s = self.conv_x(lambda p, q: torch.einsum('nkhw,ncijhw->kcij', p, q), DL,
                        F.pad(A, (pad, pad, pad, pad)).unfold(2, Ho, 1).unfold(3, Wo, 1), N * Ho * Wo)
        self.put(dw, (K, C, kh, kw), (C * kh * kw, kh * kw, kw, 1),
                 add(self.vec(dw, K * C * kh * kw).map(lambda t: t.view(K, C, kh, kw)), s), 'f32')
        self.put(db, (K,), (1,), add(self.vec(db, K), self.chan_sum(X(DL.permute(0, 2, 3, 1).reshape(-1, K)))), 'f32')
        return 0

    # ---- add, MaxPool2d, bilinear upsampling, layout
    def segnb_add(self, dtype, a, ld_a, b, ld_b, out, ld_out, N, H, W, Cp, stream):
        dt = _name(dtype)
        ops = [self.pix(p, N, H, W, Cp, ld, dt) for p, ld in ((a, ld_a), (b, ld_b)) if p]       # a NULL operand: zeros (H:385)
        r = X(torch.zeros(N, H, W, Cp)) if not ops else (ops[0] if len(ops) == 1 else add(*ops))
        self.put_pix(out, N, H, W, Cp, ld_out, r, dt)
        return 0

    @staticmethod
    def pool_windows(x, k, st, pd):
        """[N,H,W,C] -> [N,Ho,Wo,C,k*k] with -inf outside the image, window positions a * k + b"""
        xp = F.pad(x.permute(0, 3, 1, 2), (pd, pd, pd, pd), value=float('-inf')).permute(0, 2, 3, 1)
        w = xp.unfold(1, k, st).unfold(2, k, st)
        return w.reshape(*w.shape[:4], k * k)

    def first_max(self, w):
        return self.first_of(w == w.amax(-1, keepdim=True), -1)

    def segnb_maxpool_fwd(self, dtype, x, ld_x, N, H, W, Cp, k, stride, pad, out, ld_out, idx, stream):
        dt = _name(dtype)
        w = self.pool_windows(self.pix(x, N, H, W, Cp, ld_x, dt).v, k, stride, pad)
        Ho, Wo = w.shape[1:3]
        self.put_pix(out, N, Ho, Wo, Cp, ld_out, X(w.amax(-1)), dt)
        if idx is not None:                                         # the window position a * k + b of the maximum (H:403)
            pos = (self.first_max(w) * torch.arange(k * k)).sum(-1)
            self.put(idx, (N, Ho, Wo, Cp), (Ho * Wo * Cp, Wo * Cp, Cp, 1), X(pos), 'u8')
        return 0

    def maxpool_backward(self, dt, x, ld_x, g, N, H, W, Cp, k, st, pd, dx, ld_dx):
        first = self.first_max(self.pool_windows(self.pix(x, N, H, W, Cp, ld_x, dt).v, k, st, pd))
        Ho, Wo = first.shape[1:3]
        terms = []
        for a in range(k):
            for b in range(k):
                t = g.map(lambda q: F.pad(torch.zeros(N, H, W, Cp, dtype=torch.float64), (0, 0, pd, pd + st, pd, pd + st)))
                for dst, src in ((t.v, g.v), (t.e, g.e)):
                    dst[:, a:a + st * Ho:st, b:b + st * Wo:st] = src * first[..., a * k + b]
                terms.append(t.map(lambda q: q[:, pd:pd + H, pd:pd + W]))
        self.put_pix(dx, N, H, W, Cp, ld_dx, fsum(stack(terms), 0), dt)
        return 0

    def segnb_maxpool_bwd(self, dtype, x, ld_x, g_out, ld_go, N, H, W, Cp, k, stride, pad, dx, ld_dx, idx, stream):
        dt = _name(dtype)
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        return self.maxpool_backward(dt, x, ld_x, self.pix(g_out, N, Ho, Wo, Cp, ld_go, dt), N, H, W, Cp, k, stride, pad, dx, ld_dx)

    def segnb_maxpool_bwd_add(self, dtype, x, ld_x, g_out, ld_go, g_out2, ld_go2, N, H, W, Cp, k, stride, pad, dx, ld_dx, idx,
                              stream):
        dt = _name(dtype)
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        g = stored(add(self.pix(g_out, N, Ho, Wo, Cp, ld_go, dt), self.pix(g_out2, N, Ho, Wo, Cp, ld_go2, dt)), dt)    # R7
        return self.maxpool_backward(dt, x, ld_x, g, N, H, W, Cp, k, stride, pad, dx, ld_dx)

    @staticmethod
    def bilinear_matrix(n):
        """[2n][n]: row d holds the two weights of output d; source coordinate max((d + 0.5) / 2 - 0.5, 0)"""
        m = torch.zeros(2 * n, n, dtype=torch.float64)
        for d in range(2 * n):
            s = max((d + 0.5) / 2 - 0.5, 0.0)
            i0 = int(s)
            i1 = min(i0 + 1, n - 1)
            m[d, i0] += 1 - (s - i0)
            m[d, i1] += s - i0
        return m

    def bilinear(self, x, H, W, eq, n_terms):
        """the weights are multiples of 1/16: the second operand of conv_x carries that granularity"""
        mh, mw = self.bilinear_matrix(H), self.bilinear_matrix(W)
        return self.conv_x(lambda p, q: torch.einsum(eq, mh, p, mw) * (q * 16), x, torch.tensor(1.0 / 16, dtype=torch.float64),
                           n_terms)

    def segnb_upsample_bilinear2x_fwd(self, dtype, x, ld_x, N, H, W, Cp, out, ld_out, stream):
        dt = _name(dtype)            # 4 products and 3 additions
        self.put_pix(out, N, 2 * H, 2 * W, Cp, ld_out, self.bilinear(self.pix(x, N, H, W, Cp, ld_x, dt).v, H, W, 'ah,nhwc,bw->nabc', 7),
                     dt)
        return 0

    def segnb_upsample_bilinear2x_bwd(self, dtype, g_out, ld_go, N, H, W, Cp, dx, ld_dx, stream):
        dt = _name(dtype)            # the transpose: up to 16 products and 15 additions
        self.put_pix(dx, N, H, W, Cp, ld_dx,
                     self.bilinear(self.pix(g_out, N, 2 * H, 2 * W, Cp, ld_go, dt).v, H, W, 'ah,nabc,bw->nhwc', 31), dt)
        return 0

    def segnb_nhwc_to_nchw_f32(self, dtype, a, ld, N, H, W, C, out, stream):
        A = self.pix(a, N, H, W, C, ld, _name(dtype))
        self.put(out, (N, C, H, W), (C * H * W, H * W, W, 1), A.map(lambda t: t.permute(0, 3, 1, 2)), 'f32')
        return 0

    # ---- optimizers (torch.optim.SGD / RMSprop / Adam, H:743-748)
    def segnb_sgd_step(self, p, g, n, lr, stream):
        self.put(p, (n,), (1,), sub(self.vec(p, n), mul(X(_f32(lr)), self.vec(g, n))), 'f32')
        return 0

    def segnb_rmsprop_step(self, p, g, sq, n, lr, alpha, eps, stream):
        P, G, V = self.vec(p, n), self.vec(g, n), self.vec(sq, n)
        al = X(_f32(alpha))
        v = self.put(sq, (n,), (1,), add(mul(al, V), mul(sub(X(1.0), al), mul(G, G))), 'f32')
        self.put(p, (n,), (1,), sub(P, div(mul(X(_f32(lr)), G), add(sqrt(v), X(_f32(eps))))), 'f32')
        return 0

    def segnb_adam_step(self, p, g, m, v, n, lr, beta1, beta2, eps, step, stream):
        P, G, M, V = self.vec(p, n), self.vec(g, n), self.vec(m, n), self.vec(v, n)
        b1, b2 = X(_f32(beta1)), X(_f32(beta2))
        M = self.put(m, (n,), (1,), add(mul(b1, M), mul(sub(X(1.0), b1), G)), 'f32')
        V = self.put(v, (n,), (1,), add(mul(b2, V), mul(sub(X(1.0), b2), mul(G, G))), 'f32')
        bc1, bc2 = 1 - _f32(beta1) ** step, 1 - _f32(beta2) ** step         # "computed on the host in fp64" (H:747)
        denom = add(div(sqrt(V), cast(torch.tensor(bc2 ** 0.5, dtype=torch.float64))), X(_f32(eps)))
        self.put(p, (n,), (1,), sub(P, mul(cast(torch.tensor(_f32(lr) / bc1, dtype=torch.float64)), div(M, denom))), 'f32')
        return 0

    # ---- packers
    def segnb_pack_input_nchw(self, x, N, C, H, W, out, dtype, Cp, ld_out, stream):
        v = _mem(x, N * C * H * W, torch.float32).view(N, C, H, W).permute(0, 2, 3, 1).double()
        self.put_pix(out, N, H, W, Cp, ld_out, X(F.pad(v, (0, Cp - C))), _name(dtype))
        return 0

    def segnb_pack_input_u8(self, img, N, H, W, C, scale, mean, std, out, dtype, Cp, ld, stream):
        u = X(_mem(img, N * H * W * C, torch.uint8).view(N, H, W, C).double())
        m = X(torch.tensor([_f32(mean[i]) for i in range(C)]))
        inv = stored(div(X(1.0), X(torch.tensor([_f32(std[i]) for i in range(C)]))), 'f32')          # R11
        v = mul(sub(mul(u, X(_f32(scale))), m), inv)
        self.put_pix(out, N, H, W, Cp, ld, v.map(lambda t: F.pad(t, (0, Cp - C))), _name(dtype))
        return 0

    def segnb_pack_weight(self, w, wp, dtype, Mp, Cp, ntaps, s_m, s_c, tap_off, mmap, cmap, stream):
        """packed (mp, t, cp) = w[mmap[mp] * s_m + cmap[cp] * s_c + tap_off[t]], -1 in a map: padding, zero (H:151-152)"""
        mm, cm = _mem(mmap, Mp, torch.int32).long(), _mem(cmap, Cp, torch.int32).long()
        out = torch.zeros(Mp, ntaps, Cp, dtype=torch.float64)
        for i in range(Mp):
            for t in range(ntaps):
                for c in range(Cp):
                    if mm[i] >= 0 and cm[c] >= 0:
                        out[i, t, c] = float(_mem(int(w) + 4 * int(mm[i] * s_m + cm[c] * s_c + int(tap_off[t])), 1, torch.float32)[0])
        self.put(wp, (Mp, ntaps, Cp), (ntaps * Cp, Cp, 1), X(out), _name(dtype))
        return 0


# ------------------------------------------------------------------------------------------------ the comparison
def region(buf, note):
    return torch.as_strided(buf.reshape(-1), note.shape, note.strides)


def compare(name, got, mine, note):
    """one output buffer `got` against the oracle's buffer `mine` and its note (None: an input riding along, compared bit
    for bit) -> (exact, worst err / bound, elements left out, failure message or None)"""
    got, mine = got.detach().cpu(), mine.detach().cpu()
    if tuple(got.shape) != tuple(mine.shape) or got.dtype != mine.dtype:
        return True, 0.0, 0, '%s: %s %s vs %s %s' % (name, got.dtype, tuple(got.shape), mine.dtype, tuple(mine.shape))
    bits = (lambda t: t.view(torch.int16)) if got.dtype == torch.bfloat16 else (lambda t: t)
    if note is None:
        return True, 0.0, 0, None if torch.equal(bits(got), bits(mine)) else '%s: an input changed' % name
    a, b = got.clone(), mine.clone()
    region(a, note).zero_()
    region(b, note).zero_()
    if not torch.equal(bits(a), bits(b)):
        return note.exact, 0.0, 0, '%s: written outside its region' % name
    g = region(got, note).double()
    if note.repl:
        g = g.sum(0)
    keep = torch.ones_like(note.ref, dtype=torch.bool) if note.amb is None else ~note.amb
    left = int((~keep).sum())
    if left > MAX_LEFT_OUT * keep.numel():
        return note.exact, 0.0, left, '%s: %d of %d elements ambiguous' % (name, left, keep.numel())
    ex = keep & (note.err == 0)
    want = rnd(note.ref, note.dt)
    bad = ex & ~(g == want)                     # in float64: the tables, the int64 and uint8 outputs are compared as they are
    msg, worst = None, 0.0
    if bool(bad.any()):
        i = bad.nonzero()[:4].tolist()
        msg = '%s (exact): %d/%d elements differ, first idx %s got %s want %s' % (
            name, int(bad.sum()), bad.numel(), i, [float(g[tuple(j)]) for j in i], [float(want[tuple(j)]) for j in i])
    inx = keep & (note.err != 0)
    if msg is None and bool(inx.any()):         # note.err is the bound at the store already: no further store rounding ('f64')
        worst, msg = eb.within_bound(name, g[inx], note.ref[inx], note.err[inx] / U, 1, 'f64')
    return note.exact, worst, left, msg


def compare_case(outs_got, outs_mine, notes):
    """-> (every output exact, worst ratio, elements left out, list of failure messages)"""
    assert sorted(outs_got) == sorted(outs_mine), (sorted(outs_got), sorted(outs_mine))
    exact, worst, left, msgs = True, 0.0, 0, []
    for k in sorted(outs_mine):
        e, w, l, m = compare(k, outs_got[k], outs_mine[k], notes.get(outs_mine[k].data_ptr()))
        exact, worst, left = exact and e, max(worst, w), left + l
        if m:
            msgs.append(m)
    return exact, worst, left, msgs


# ------------------------------------------------------------------------------------------------ running a case
class one_thread(object):
    """the tensors are a few thousand elements: torch's thread pool costs ten times what it saves"""
    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *exc):
        torch.set_num_threads(self.n)


def run_backend(backend, fn, *args):
    """fn(*args) with `backend` installed (None: the library) -> its result; the previous backend is put back"""
    from segnb import _native as nv
    before = nv._test_backend
    nv.set_backend_for_testing(backend)
    try:
        with one_thread():
            return fn(*args)
    finally:
        nv.set_backend_for_testing(before)


def oracle_outputs(fn, *args, **kw):
    """-> (output buffers of the oracle's run on the CPU, its notes, the oracle)"""
    o = kw.get('oracle') or Oracle()
    outs = run_backend(o, fn, *args)
    return outs, o.notes, o


def check_left_out(notes):
    """the 1 % cap on the oracle alone -> list of (pointer, left out, of)"""
    bad = []
    for p, n in notes.items():
        if n.amb is not None and int(n.amb.sum()) > MAX_LEFT_OUT * n.amb.numel():
            bad.append((p, int(n.amb.sum()), n.amb.numel()))
    return bad


class Recorder(object):
    """per (row, dtype): exact, worst err / bound, elements left out; written only from a complete run, on request"""
    def __init__(self, section, expected):
        self.section, self.expected, self.rows = section, set(expected), {}

    def add(self, key, exact, worst, left):
        self.rows[key] = (exact, worst, left)

    def write(self, path):
        if set(self.rows) != self.expected:
            return False
        keep = []
        if os.path.exists(path):
            with open(path) as f:
                text = f.read()
            keep = [b for b in text.split('## ')[1:] if not b.startswith(self.section + '\n')]
        block = self.section + '\n' + ''.join('%-44s %-7s worst err/bound %.4f  left out %d\n' % (
            k, 'exact' if e else 'bound', w, l) for k, (e, w, l) in sorted(self.rows.items()))
        with open(path, 'w') as f:
            f.write('# tests/test_ew_oracle_gpu.py and tests/test_ew_errbound_gpu.py on MI355X (SEGNB_RECORD_EWORACLE=1): per case,\n'
                    '# whether every output is exact (compared with ==), the worst err / bound of the others, elements left out.\n'
                    '# Measurements: the thresholds of the tests are == and 1.\n')
            for b in sorted(keep + [block]):
                f.write('## ' + b)
        return True
