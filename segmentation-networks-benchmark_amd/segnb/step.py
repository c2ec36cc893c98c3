"""The protocol around a step's launches, once for both schedulers (lib.models.zf_unet._ZFUnetPlan, segnb.net.HipNet / Tape).

A step is launched from Python while the library records its ABI calls (segnb.launchlist); later steps of the same key
replay the lists from C (3-4 us of host time per launch instead of the 10-14 us of a ctypes call).  A list is valid only while
every pointer in it is: same buffers, same streams, same mode (``list_key``: the part of that every owner needs); whatever
varies between steps enters through persistent buffers, and host code that must run between launches cuts the list.
WHICH step records, what else is in a key and what a step launches stay with each owner."""
import contextlib
import os

import torch

from .launchlist import Recorder

USE_LISTS = os.environ.get('SEGNB_CPLAN', '1') != '0'       # (the default of each owner's use_cplan)
KINDS = ('fwd', 'bwd')


class Entry(dict):
    """One key's recorded lists ('fwd' / 'bwd') and whatever its owner keeps beside them.  'state': 'new' (never run), 'seen'
    (ran eagerly), 'fwd' (a forward list waits for its backward), 'ready' (replayable), 'eager' (for good: holds no list).
    bench.py is a reader: ``p[0]`` (truthy when a list is held) of ZF_UNET's entries, ``.get('state')`` of the executor's."""

    def __getitem__(self, k):
        if k == 0:
            return next((self[n] for n in KINDS if self.get(n) is not None), None)
        return dict.__getitem__(self, k)

    def drop(self):           # (frees the lists; the state is the caller's)
        for kind in KINDS:
            lst = self.pop(kind, None)
            if lst is not None:
                lst.destroy()


class StepCache(dict):
    """key -> Entry"""

    def entry(self, key):
        ent = self.get(key)
        if ent is None:
            ent = self[key] = Entry(state='new')
        return ent

    @staticmethod
    @contextlib.contextmanager
    def recording(ent, kind):
        """Record the launches of the body, which gets the Recorder and stores ``ent[kind] = rec.finish()``.  A body that raises,
        makes a call the library refuses or declines its list stores none: the entry is then eager for good and its lists are
        freed.  Yields None, and records nothing, for such an entry and for ent None."""
        if ent is None or ent['state'] == 'eager':
            yield None
            return
        with Recorder() as rec:
            try:
                yield rec
            finally:
                if ent.get(kind) is None:
                    ent.drop()
                    ent['state'] = 'eager'


def list_key(rt, flat, hook, enabled):
    """What every list depends on: both queues, the flat parameter / gradient storage, the module buffers, whether a
    gradient-ready hook cuts the backward.  None: no lists (switched off, or not on a GPU)."""
    if not enabled or rt.device.type != 'cuda':
        return None
    side = rt.side_stream()
    return (rt.stream, side.cuda_stream if side is not None else 0, flat.flat_p.data_ptr(), flat.flat_g.data_ptr(),
            tuple(b.data_ptr() for b in flat.buffer_list()), hook is not None)


def ready_hook(module, only_active=False):
    """The data-parallel "gradients ready" hook; only_active: None as well while its owner is switched off."""
    hook = getattr(module, '_grad_ready_hook', None)
    if hook is not None and only_active and not getattr(getattr(hook, '__self__', None), 'active', True):
        return None
    return hook


def values_stamp(flat):
    """Changes whenever a parameter value may have (an in-place update, new flat storage): packed weights are as old as it."""
    return (sum(p._version for p in flat.param_list()), flat.version, flat.flat_p.data_ptr())


def set_compute_dtype(module, dtype, slot):
    """'bf16' = throughput path, 'f32' = exact-fp32 MFMA parity path; a change drops the engine kept in module.<slot>."""
    if dtype not in ('bf16', 'f32'):
        raise ValueError("compute dtype must be 'bf16' or 'f32'")
    if dtype != module.compute_dtype:
        module.compute_dtype = dtype
        setattr(module, slot, None)
    return module


def check_channels(x, cin, cdim=1):
    if x.dim() != 4 or x.shape[cdim] != cin:
        raise ValueError('expected input [N, %d, H, W] (float) or [N, H, W, %d] (uint8), got %s %s'
                         % (cin, cin, x.dtype, tuple(x.shape)))


def enter(module, slot, x, make):
    """-> (the module's one engine, made for x's device; x as the engine reads it: uint8 NHWC kept, anything else fp32)"""
    eng = getattr(module, slot)
    if eng is None or eng.rt.device != x.device:
        eng = make(x.device)
        setattr(module, slot, eng)
    x = x.detach().contiguous()
    return eng, x if x.dtype == torch.uint8 else x.float()


def stage_dlogits(dlogits, buf):
    """d(loss)/d(logits) where a recorded list reads it (autograd hands over a new tensor; a loss may have written there)."""
    if buf is None:
        buf = torch.empty_like(dlogits)
    if dlogits.data_ptr() != buf.data_ptr():
        buf.copy_(dlogits)
    return buf


def run_backward(module, rt, flat, train, has_bn, lists, aliased=False):
    """One backward: lists(accumulate_in_place) launches it.  Directly delivered weight gradients are STORED when the gradient
    buffer was just cleared, ADDED when gradients accumulate in place or the forward saw .grad aliasing it (`aliased`)."""
    if not train and has_bn():
        # the backward implements the TRAINING-mode BatchNorm gradient (batch statistics); through an eval-mode forward
        # (running statistics) BatchNorm is a plain affine map and that formula is wrong
        raise RuntimeError('backward through an eval-mode forward is not supported: BatchNorm gradients are '
                           'implemented for training mode (call model.train(), or run the forward under no_grad)')
    acc = flat.begin_backward()
    with rt.weight_grads(store=not acc and not aliased):
        lists(acc)
    hook = getattr(module, '_grad_sync_hook', None)
    if hook is not None:
        hook(flat)
    # gradients live in ONE flat buffer; parameter.grad tensors are views of it (installed here, not returned through
    # autograd, so they never get cloned and a flat optimizer / all-reduce can run)
    flat.publish_grads(acc)
