"""Autograd functions over the multi-class loss kernels (segnb_mc_loss_*, csrc/mc_loss.hip; include/segnb_mc_loss.h).

One streaming pass over (logits fp32 NCHW [N,C,H,W], target int64 [N,H,W]) produces the global sums of every multi-class
term (focal, weighted NLL, per-class smooth Jaccard); the finalize turns them into the loss and the per-class derivatives on
the device (no host sync); a second pass writes d(loss)/d(logits) scaled by the upstream gradient.  On one device the
reduction and the finalize are ONE launch (the last workgroup finalizes); a data-parallel job all-reduces the 3C + 8 sums
between the two launches (seglosses.DataParallelHooks), so means use the global pixel counts.

Unlike the binary family there is no metric cache (seglosses._remember): the binary metrics never answer from these sums.
"""
import torch

from . import _native as nv
from .seglosses import DataParallelHooks, _grad_buffer_for, _stream

CFG_FIELDS = ('mode', 'ignore_index', 'gamma', 'w_focal', 'w_nll', 'w_jaccard', 'norm', 'focal_mean', 'reduce')

# _ONE_LAUNCH = False (module attribute): segnb_mc_loss_reduce + segnb_mc_loss_finalize as two launches (A/B, tests)
_ONE_LAUNCH = True
_work = {}      # (device index, stream, C) -> the work buffer of segnb_mc_loss_reduce*: zeroed once, left ready by every launch


def make_cfg(mode=0, ignore_index=-100, gamma=2.0, w_focal=0.0, w_nll=0.0, w_jaccard=0.0, norm=1.0, focal_mean=1, reduce=1):
    return (int(mode), int(ignore_index), float(gamma), float(w_focal), float(w_nll), float(w_jaccard), float(norm),
            int(focal_mean), int(reduce))


def _cspec(C, cfg, nll_w, jac_w):
    s = nv.McLossSpec()
    s.C = C
    for k, v in zip(CFG_FIELDS, cfg):
        setattr(s, k, v)
    s.nll_weight = nv.ptr(nll_w)
    s.jac_weight = nv.ptr(jac_w)
    return s


def _prep(logits, target):
    if logits.dim() != 4 or target.dim() != 3 or target.shape != (logits.shape[0],) + tuple(logits.shape[2:]):
        raise ValueError('logits [N,C,H,W] %s and target [N,H,W] %s do not match' % (tuple(logits.shape), tuple(target.shape)))
    C = logits.shape[1]
    if not 1 <= C <= 256:
        raise ValueError('the multi-class losses support 1..256 classes, got %d' % C)
    x = logits.detach().contiguous().float()
    t = target.detach()
    if t.dtype != torch.int64:
        t = t.to(torch.int64)
    return x, t.contiguous()


def _weight(w, x):
    if w is None:
        return None
    w = w.detach().to(device=x.device, dtype=torch.float32).contiguous()
    if w.numel() != x.shape[1]:
        raise ValueError('%d class weights for %d classes' % (w.numel(), x.shape[1]))
    return w


def _work_for(x, C, st):
    key = (x.device.index, st, C)
    work = _work.get(key)
    if work is None:
        work = _work[key] = torch.zeros(int(nv.query('segnb_mc_loss_work_doubles', C)), dtype=torch.float64, device=x.device)
    return key, work


def reduce_finalize(x, t, cfg, nll_w, jac_w):
    """-> fin fp32[8 + 3C] on the device (layout: include/segnb_mc_loss.h)."""
    N, C, H, W = x.shape
    fin = torch.empty(8 + 3 * C, dtype=torch.float32, device=x.device)
    st = _stream(x)
    cs = _cspec(C, cfg, nll_w, jac_w)
    key, work = _work_for(x, C, st)
    try:
        if DataParallelHooks.sums_allreduce is None and _ONE_LAUNCH:
            nv.call('segnb_mc_loss_reduce_finalize', nv.ptr(x), nv.ptr(t), N, H * W, cs, nv.ptr(work), nv.ptr(fin), st)
            return fin
        sums = torch.empty(3 * C + 8, dtype=torch.float64, device=x.device)
        nv.call('segnb_mc_loss_reduce', nv.ptr(x), nv.ptr(t), N, H * W, cs, nv.ptr(work), nv.ptr(sums), st)
    except BaseException:
        # a launch that failed may have left a ticket drawn: the next loss on this stream starts from a fresh, zeroed buffer
        _work.pop(key, None)
        raise
    if DataParallelHooks.sums_allreduce is not None:
        DataParallelHooks.sums_allreduce(sums)
    nv.call('segnb_mc_loss_finalize', nv.ptr(sums), cs, nv.ptr(fin), st)
    return fin


class McLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, cfg, nll_w, jac_w):
        x, t = _prep(logits, target)
        nll_w, jac_w = _weight(nll_w, x), _weight(jac_w, x)
        fin = reduce_finalize(x, t, cfg, nll_w, jac_w)
        ctx.cfg = cfg
        ctx.weights = (nll_w, jac_w)
        ctx.save_for_backward(x, t, fin)
        McLossFn.last_fin = fin
        C = x.shape[1]
        return fin[0] if cfg[8] else fin[8:8 + C]     # (views of this call's own result vector: no copy launch)

    @staticmethod
    def backward(ctx, gout):
        x, t, fin = ctx.saved_tensors
        nll_w, jac_w = ctx.weights
        g = gout.detach().contiguous().float()
        if DataParallelHooks.grad_scale != 1.0:
            g = g * DataParallelHooks.grad_scale
        dx = _grad_buffer_for(x)
        if dx is None:
            dx = torch.empty_like(x)
        N, C, H, W = x.shape
        nv.call('segnb_mc_loss_bwd', nv.ptr(x), nv.ptr(t), N, H * W, _cspec(C, ctx.cfg, nll_w, jac_w), nv.ptr(fin), nv.ptr(g),
                nv.ptr(dx), _stream(x))
        return dx, None, None, None, None


def mc_loss(logits, target, cfg, nll_weight=None, jac_weight=None):
    """The multi-class loss of `cfg` (make_cfg): a 0-dim tensor, or the [C] per-class Jaccard vector when cfg reduce = 0.
    ``mc_loss.last_fin`` is the full result vector of the call (counts of valid / all pixels and bad labels at 3, 4, 5)."""
    out = McLossFn.apply(logits, target, cfg, nll_weight, jac_weight)
    mc_loss.last_fin = McLossFn.last_fin
    McLossFn.last_fin = None
    return out


mc_loss.last_fin = None
