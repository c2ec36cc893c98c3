"""The BatchNorm pass layer: the ONE place that names a segnb_bn_* / segnb_head_bn_* entry point.

BnLayer holds what one BatchNorm (+ activation) layer owns (buffers, activation, accessors for parameters and gradient targets)
and turns "this situation" into "this entry point with this argument list".  Policy stays with the callers (Stage, conv_unit,
bn_act, InPlaceABN): whether a layer is direct / recomputed / lazy, when a fork is armed, side streams.  Views: engine.View.
"""
import os

import torch

from . import _native as nv

BN_EPS, BN_MOMENTUM = 1e-5, 0.1
STAT_REPLICAS = 16     # SEGNB_STAT_REPLICAS

# BatchNorm finalize folded into the activation / apply launches of a differentiated training forward (segnb_bn_fwd_fused /
# _bwd_apply_fused): one launch less per layer and direction -- for ZF_UNET 44 launches of ~5 us less on the dependent chain
# (re-measured after the convolutions got faster: 5.71 -> 5.58 ms/step; neutral when first tried, 7.47 vs 7.39 ms/step: every
# block of the big kernel starts with the same dependent statistics loads).  A/B: SEGNB_FUSE_FINALIZE=0
FUSE_FINALIZE = os.environ.get('SEGNB_FUSE_FINALIZE', '1') != '0'


def _pl(v):           # (address, pixel stride) of an optional View
    return (None, 0) if v is None else (v.ptr, v.ld)


def _dp(t):
    return nv.ptr(None if t is None else t.detach())


def module_params(bn, eps=None, momentum=None):
    """-> the params accessor of a torch BatchNorm-like module (its own eps / momentum unless given)"""
    eps = float(getattr(bn, 'eps', BN_EPS)) if eps is None else eps
    momentum = float(getattr(bn, 'momentum', BN_MOMENTUM) or BN_MOMENTUM) if momentum is None else momentum
    return lambda: (bn.weight, bn.bias, bn.running_mean, bn.running_var, getattr(bn, 'num_batches_tracked', None), eps, momentum)


def stats_into(code, stream, v, out_stats):
    """statistics of View v into the channel range out_stats = (table, element offset, row stride)"""
    nv.call('segnb_bn_stats_ld', code, v.ptr, v.ld, v.N, v.H, v.W, v.Cp, nv.ptr(out_stats[0], out_stats[1]), out_stats[2], stream)


class BnLayer(object):
    """params() -> (gamma, beta, running_mean, running_var, num_batches_tracked or None, eps, momentum); gamma may be an
    "effective gamma" tensor (InPlaceABN's |w| + eps).  None: a layer WITHOUT BatchNorm (activation only; its sums are the bias
    gradient).  grads() -> the two fp32 gradient targets (dgamma, dbeta); accumulate: added to (1) or overwritten (0).
    zeros(shape, dtype) allocates the layer's device buffers."""

    def __init__(self, C, Cp, zeros, act, slope, params=None, grads=None, accumulate=1):
        self.C, self.Cp, self.act, self.slope, self.params, self.grads, self.accumulate = C, Cp, act, slope, params, grads, accumulate
        self.stats = zeros((STAT_REPLICAS, 2, Cp), torch.float64)      # consumed + re-zeroed by segnb_bn_finalize (or the fused applies)
        self.sums = zeros((STAT_REPLICAS, 2, Cp), torch.float64)       # consumed + re-zeroed by segnb_bn_bwd_finalize (or its fused forms)
        self.coef, self.bcoef = zeros((4, Cp), torch.float32), zeros((3, Cp), torch.float32)
        # stats_left: a fused forward left the forward statistics for this layer's backward to clear (if that backward never
        # runs, the owner clears them before the next forward accumulates on top); fused_fwd: the last forward was a fused one
        self.stats_left = self.fused_fwd = False

    def _geom(self, code, y, with_c=True):
        return (code, y.ptr, y.ld, y.N, y.H, y.W) + ((self.C, self.Cp) if with_c else (self.Cp,))

    def _fwd_params(self, *lead):
        gamma, beta, rm, rv, nbt, eps, mom = self.params()
        return lead + (_dp(gamma), _dp(beta), eps, mom, nv.ptr(rm), nv.ptr(rv), nv.ptr(nbt))

    def _bwd_params(self, clear_stats=True):
        dgamma, dbeta = self.grads()
        if clear_stats:
            self.stats_left = False
        return (nv.ptr(self.coef), nv.ptr(self.sums), _dp(self.params()[0]), nv.ptr(self.bcoef), nv.ptr(dgamma), nv.ptr(dbeta),
                self.accumulate, nv.ptr(self.stats) if clear_stats else None)

    def _coef(self):
        return self.coef if self.params is not None else None

    def producer(self, y):
        """-> the (y, coef, sums, act, slope) a data-gradient launch needs to do THIS layer's backward reduction in its epilogue
        (coef None without BatchNorm: it stores dz = g * act'(a) and sums it).  The caller checks that the layer qualifies."""
        return (y, self._coef(), self.sums, self.act, self.slope)

    # ---- statistics / finalize -------------------------------------------------------------------------------
    def stats_of(self, code, stream, x):
        nv.call('segnb_bn_stats', code, x.ptr, x.ld, x.N, x.H, x.W, self.Cp, nv.ptr(self.stats), stream)

    def finalize(self, stream, count, train):
        """statistics (train) or running statistics -> coef; consumes and re-zeroes the statistics"""
        nv.call('segnb_bn_finalize', *(self._fwd_params(nv.ptr(self.stats), self.C, self.Cp, float(count))
                                       + (1 if train else 0, nv.ptr(self.coef), stream)))

    def finalize_keep(self, stream, count):
        """the fused forward's finalize WITHOUT its activation pass (the consumer applies coef while it loads)"""
        nv.call('segnb_bn_finalize_keep', *(self._fwd_params(nv.ptr(self.stats), self.C, self.Cp, float(count))
                                            + (nv.ptr(self.coef), nv.ptr(self.sums), stream)))
        self.stats_left = self.fused_fwd = True

    # ---- forward activation pass -------------------------------------------------------------------------------
    def act_fwd(self, code, stream, y, out, coef, act, slope, dropmul=None, pool_out=None, up_out=None, res=None):
        nv.call('segnb_bn_act_fwd', *(self._geom(code, y, False) + (nv.ptr(coef), act, slope, nv.ptr(dropmul)) + _pl(out)
                                      + _pl(pool_out) + _pl(up_out) + _pl(res) + (stream,)))

    def forward(self, code, stream, y, fused, train=True, dropmul=None, out=None, pool_out=None, up_out=None, res=None,
                out_stats=None, stats_src=None, head=None):
        """BatchNorm (batch statistics when train) + activation (+ Dropout2d multipliers, + residual) of y -> out [+ 2x2 max-pooled
        / nearest-x2 copies].  fused: the finalize is folded into the pass -- the statistics stay for this layer's backward to
        clear (stats_left), the backward sums are cleared here (include/segnb_hip.h); stats_src = (table, element offset, row stride):
        the statistics are that range of a concat buffer's table (nobody's backward owns them); head = (weight, bias, K, logits):
        the 1x1 classifier runs on the activated values in the same launch.  out_stats: the pass that writes `out` also sums it into
        that range where an entry point does (unfused, no pooled / residual operands): returns True then (else: stats_into)."""
        self.fused_fwd = bool(fused)
        if fused or head is not None:
            tail = (nv.ptr(self.coef), nv.ptr(self.sums), self.act, self.slope, nv.ptr(dropmul)) + _pl(out)
        if head is not None:
            head_w, head_b, K, logits = head
            nv.call('segnb_bn_fwd_fused_head', *(self._geom(code, y) + self._fwd_params(nv.ptr(self.stats)) + tail
                                                 + (nv.ptr(head_w), nv.ptr(head_b), K, nv.ptr(logits), stream)))
            self.stats_left = True
        elif fused and stats_src is not None:
            nv.call('segnb_bn_fwd_fused_ld', *(self._geom(code, y) + self._fwd_params(nv.ptr(stats_src[0], stats_src[1]), stats_src[2])
                                               + tail + (stream,)))
        elif fused:
            nv.call('segnb_bn_fwd_fused', *(self._geom(code, y) + self._fwd_params(nv.ptr(self.stats)) + tail + _pl(pool_out)
                                            + _pl(up_out) + _pl(res) + (stream,)))
            self.stats_left = True
        else:
            if self.params is not None:
                self.finalize(stream, y.N * y.H * y.W, train)
            if out_stats is not None and pool_out is None and up_out is None and res is None:
                nv.call('segnb_bn_act_fwd_stats', *(self._geom(code, y, False) + (nv.ptr(self._coef()), self.act, self.slope, nv.ptr(dropmul))
                                                    + _pl(out) + (nv.ptr(out_stats[0], out_stats[1]), out_stats[2], stream)))
                return True
            self.act_fwd(code, stream, y, out, self._coef(), self.act, self.slope, dropmul, pool_out, up_out, res)
        return False

    # ---- backward reduction ------------------------------------------------------------------------------------
    def reduce(self, code, stream, y, g=None, g2=None, g_pool=None, g_up=None, dropmul=None, dz=None, store=True, res=None):
        """dz = act'(y) * (sum of the gradient sources: g [+ g2], pooled, upsampled) and its two per-channel sums.  store False
        (or no dz): sums only -- the apply pass recomputes dz.  Two direct sources go to the _add form instead of an add pass."""
        head = self._geom(code, y, False) + (nv.ptr(self._coef()), self.act, self.slope, nv.ptr(dropmul))
        dzp = (dz.ptr if store else None, dz.ld) if dz is not None else (None, 0)
        if g2 is not None:
            nv.call('segnb_bn_act_bwd_reduce_add', *(head + _pl(g) + _pl(g2) + dzp + (nv.ptr(self.sums),) + _pl(res) + (stream,)))
        else:
            nv.call('segnb_bn_act_bwd_reduce', *(head + _pl(g) + _pl(g_pool) + _pl(g_up) + dzp + (nv.ptr(self.sums),) + _pl(res)
                                                 + (stream,)))

    def head_reduce(self, code, stream, y, dropmul, head_w, K, dlogits, dz, store, dw, db):
        """d(logits) through the 1x1 classifier (+ its dw, db), the activation / Dropout2d and this layer's reduction in one pass"""
        nv.call('segnb_head_bn_bwd', *(self._geom(code, y) + (nv.ptr(self.coef), self.act, self.slope, nv.ptr(dropmul), nv.ptr(head_w),
                                                                K, nv.ptr(dlogits), dz.ptr if store else None, dz.ld, nv.ptr(self.sums),
                                                                nv.ptr(dw), nv.ptr(db), stream)))

    # ---- backward apply ----------------------------------------------------------------------------------------
    def apply(self, code, stream, y, dy, fused, g=None, dz=None, acc=False, src=None, head=None, clear_stats=True):
        """dy = the gradient in front of the BatchNorm, from the completed sums; dgamma / dbeta to grads().  The gradient behind
        the activation comes from ONE of: head = (weight, K, dlogits) -- recomputed from d(logits) and y; g -- the single direct
        source, dz = act'(y) * g recomputed (the *_direct forms); src = (dropmul, g_direct, g_pool, g_up) -- recomputed from the
        re-read sources; dz -- the stored tensor.  fused: the backward finalize is folded in, and the launch clears the forward
        statistics the fused forward left (clear_stats False: they were cached prefix statistics).  acc: dy is an existing
        gradient the result is added to."""
        if not fused:
            self.bwd_finalize(stream, y.N * y.H * y.W)
            # d(loss)/d(conv bias) under training-mode BatchNorm is identically zero (BN subtracts the batch mean):
            # sum(dy) = A*(sum dz - n*mean(dz) - mean(dz*yhat)*sum(yhat)) = 0.  The reference's fp32 value is pure
            # summation noise (~1e-7 of the weight-gradient scale); the flat gradient buffer already holds 0 (dbias = None).
            if g is not None:
                nv.call('segnb_bn_bwd_apply_direct', *(self._geom(code, y, False) + (nv.ptr(self.coef), nv.ptr(self.bcoef), self.act,
                                                                                     self.slope) + _pl(g) + _pl(dy) + (None, self.C, stream)))
            else:
                nv.call('segnb_bn_bwd_apply', *(self._geom(code, y, False) + (nv.ptr(self.coef), nv.ptr(self.bcoef)) + _pl(dz) + _pl(dy)
                                                + (None, self.C, stream)))
            return
        args = self._geom(code, y) + self._bwd_params(clear_stats)
        if head is not None:
            dropmul, head_w, K, dlogits = head
            name, args = 'segnb_head_bn_bwd_apply', args + (self.act, self.slope, nv.ptr(dropmul), nv.ptr(head_w), K, nv.ptr(dlogits))
        elif g is not None:
            name, args = 'segnb_bn_bwd_apply_fused_direct', args + (self.act, self.slope) + _pl(g)
        elif src is not None:
            name = 'segnb_bn_bwd_apply_fused_src'
            args += (self.act, self.slope, nv.ptr(src[0])) + _pl(src[1]) + _pl(src[2]) + _pl(src[3])
        else:
            name, args = 'segnb_bn_bwd_apply_fused', args + _pl(dz)
        nv.call(name + ('_acc' if acc else ''), *(args + _pl(dy) + (stream,)))

    def bwd_finalize(self, stream, count, gbias=None, clear_stats=False):
        """sums -> bcoef (+ dgamma / dbeta); consumes and re-zeroes the sums.  Without BatchNorm dy = dz and the sum of dz is the
        bias gradient gbias (through the dbeta slot).  clear_stats: also clears the statistics a fused forward left (no apply follows)."""
        if self.params is None:
            nv.call('segnb_bn_bwd_finalize', nv.ptr(self.sums), self.C, self.Cp, float(count), None, nv.ptr(self.coef),
                    nv.ptr(self.bcoef), None, nv.ptr(gbias), 1, stream)
            return
        dgamma, dbeta = self.grads()
        args = (nv.ptr(self.sums), self.C, self.Cp, float(count), _dp(self.params()[0]), nv.ptr(self.coef), nv.ptr(self.bcoef),
                nv.ptr(dgamma), nv.ptr(dbeta), self.accumulate)
        if clear_stats:
            nv.call('segnb_bn_bwd_finalize_clear', *(args + (nv.ptr(self.stats), stream)))
            self.stats_left = False
        else:
            nv.call('segnb_bn_bwd_finalize', *(args + (stream,)))
