"""debug tool: the ABI traffic of one training step on the ABI emulator (CPU), as text that two checkouts can diff.

    python tools/abi_call_trace.py CASE [CHECKOUT]      CASE: zf_f32 zf_f32_segw zf_bf16 zf_bf16_segw zf_bf16_segf
                                                              linknet tiramisu unet16 gcn34 squeezenet (bf16), or all
    further cases (the BatchNorm branches a default training step never takes): zf_bf16_drop (Dropout2d 0.2), zf_bf16_src
    (Stage.recompute_dz_min_mb tiny), zf_bf16_headdz (Stage.head_dz_recompute off), tiramisu_nocache (cache_prefix_stats off),
    every case above + _nofuse (BatchNorm finalize not fused), zf_bf16_eval / linknet_eval (eval-mode forward under no_grad),
    abn (InPlaceABN on its own: forward + backward, training and eval mode, both affine forms),
    zf_bf16_lists / unet16_lists / linknet_lists: three consecutive training steps with the recording path forced on (the plan
    entry points are tests/fake_plans.py's; segnb_plan_* calls are printed too, and a `--- step N` line between steps): what
    the recording step and the replayed step execute NEXT TO the lists

CHECKOUT is the repository root whose segnb.engine is traced (default: this one), so the same file traces a parent's
checkout.  Every nv.call / nv.query is printed in order; a tensor address becomes (ordinal of its storage by first
appearance, byte offset), a ctypes struct the tuple of its fields, an int array a tuple.  Every PackTable prints its
decoded rows, singles and deferred jobs.  Host-side refactors of the engine must leave this text unchanged."""
import bisect
import ctypes
import gc
import os
import sys

BASE = ('zf_f32', 'zf_f32_segw', 'zf_bf16', 'zf_bf16_segw', 'zf_bf16_segf', 'linknet', 'tiramisu', 'unet16', 'gcn34', 'squeezenet')
CASES = (BASE + ('zf_bf16_drop', 'zf_bf16_src', 'zf_bf16_headdz', 'tiramisu_nocache') + tuple(c + '_nofuse' for c in BASE)
         + ('zf_bf16_eval', 'linknet_eval', 'abn', 'zf_bf16_lists', 'unet16_lists', 'linknet_lists'))
root = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [root, os.path.join(root, 'segmentation-networks-benchmark_amd'), os.path.join(root, 'tests')]
os.environ['SEGNB_TEST_HARNESS'] = '1'       # a tool, not the product: allowed to install the emulator
import numpy as np
import torch
from segnb import _native as nv
import segnb.engine as E
import segnb.net as NET

starts, spans, ordinals, keep = [], {}, {}, []      # storage bases (sorted), base -> bytes, base -> ordinal, references


def reg(t):
    if torch.is_tensor(t):
        st = t.untyped_storage()
        if st.data_ptr() not in spans and st.nbytes():
            bisect.insort(starts, st.data_ptr())
            spans[st.data_ptr()] = st.nbytes()
            keep.append(t)             # (kept alive: no address is reused within a trace)


def addr(a):
    """(storage ordinal, byte offset) of a device address"""
    for scan in (False, True):
        if scan:                       # an address nothing passed through nv.ptr: look at every live tensor once
            for o in gc.get_objects():
                reg(o)
        i = bisect.bisect_right(starts, a) - 1
        if i >= 0 and a < starts[i] + spans[starts[i]]:
            return (ordinals.setdefault(starts[i], len(ordinals)), a - starts[i])
    return ('?',)


def norm(a):
    if isinstance(a, bool) or a is None or isinstance(a, (float, bytes, str)):
        return a
    if isinstance(a, int):
        return addr(a) if a >= (1 << 32) else a
    if torch.is_tensor(a):
        reg(a)
        return addr(a.data_ptr())
    if isinstance(a, ctypes.Structure):
        n = getattr(a, 'ntaps', None)
        out = []
        for f, _ in a._fields_:
            v = getattr(a, f)
            out.append(tuple(v[:n]) if isinstance(v, ctypes.Array) else norm(v))
        return (type(a).__name__,) + tuple(out)
    if isinstance(a, ctypes.Array):
        return tuple(a)
    if isinstance(a, (list, tuple)):
        return tuple(norm(v) for v in a)
    return type(a).__name__


OUT = []


def install(out):
    orig_ptr, orig_call, orig_query, orig_vptr, orig_init = nv.ptr, nv.call, nv.query, E.View.ptr.fget, E.PackTable.__init__

    def call(name, *args):
        out.append('%s%r' % (name, tuple(norm(a) for a in args)))
        orig_call(name, *args)

    def query(name, *args):
        r = orig_query(name, *args)
        out.append('%s%r -> %r' % (name, tuple(norm(a) for a in args), r))
        return r

    def init(self, rt, jobs, *a, **kw):
        for j in jobs:
            for v in j.values():
                reg(v)
        orig_init(self, rt, jobs, *a, **kw)
        for label, tab, dt, ptrs in (('tiled', self.table, E.PACK_JOB_DTYPE, ('w', 'packed', 'mmap', 'cmap')),
                                     ('elem', self.etable, E.PACK_JOB_DTYPE, ('w', 'packed', 'mmap', 'cmap')),
                                     ('pair', self.ptable, E.PACK_PAIR_DTYPE, ('w', 'pf', 'pd'))):
            for r in (np.frombuffer(tab.cpu().numpy().tobytes(), dtype=dt) if tab is not None else ()):
                out.append('PackTable %s %s' % (label, [(f, addr(int(r[f])) if f in ptrs and int(r[f]) else r[f].tolist())
                                                        for f in dt.names]))
        for label, js in (('singles', self.singles), ('deferred', self.deferred)):
            out.append('PackTable %s %s' % (label, [sorted((k, norm(v)) for k, v in j.items()) for j in js]))

    nv.ptr = lambda t, offset_elems=0: (reg(t), orig_ptr(t, offset_elems))[1]
    nv.call, nv.query, E.PackTable.__init__ = call, query, init
    E.View.ptr = property(lambda self: (reg(self.t), orig_vptr(self))[1])


def make(case, nocache=False):
    """-> (model, x, y, dtype)"""
    import model_checks as mc
    golden = os.path.join(root, 'tests', 'golden')
    if case.startswith('zf_'):
        from lib.models.zf_unet import ZF_UNET
        g = np.load(os.path.join(golden, 'zf_unet_tiny.npz'))
        torch.manual_seed(3)
        return (ZF_UNET(dropout_val=0.2 if case.endswith('_drop') else 0.0, filters=4), torch.from_numpy(g['x']),
                torch.from_numpy(g['y']), case.split('_')[1])
    if case == 'gcn34':
        import test_gcn_cpu as tg
        g = tg.load_case('k1')
        return tg.make_gcn('k1', g), torch.from_numpy(g['x']), torch.from_numpy(g['y']), 'bf16'
    if case == 'squeezenet':
        import test_squeezenet_cpu as ts
        g = ts.load_case('sq')
        return ts.make_squeezenet(g), torch.from_numpy(g['x']), torch.from_numpy(g['y']), 'bf16'
    if case == 'tiramisu':
        from lib.models.tiramisu import FCDenseNet
        FCDenseNet.cache_prefix_stats = not nocache
        m, _, x, y = mc.make_tiramisu(np.load(os.path.join(golden, 'tiramisu_small.npz')))
    else:
        m, _, x, y = {'linknet': mc.make_linknet, 'unet16': mc.make_unet16}[case]()
    return m, x, y, 'bf16'


def trace_abn():
    """InPlaceABN called on its own (not through an executor): forward + backward in training and eval mode, both affine forms"""
    from lib.modules.abn import InPlaceABN
    for training in (True, False):
        for form in ('gamma', 'abs_eps'):
            torch.manual_seed(7)
            m = InPlaceABN(5, affine_form=form).train(training)
            x = torch.randn(1, 5, 4, 4, requires_grad=True)
            m(x).sum().backward()


def trace(case):
    from lib.losses import BCEWithLogitsLossAndSmoothJaccard
    base = case
    for suffix in ('_nofuse', '_eval', '_drop', '_src', '_headdz', '_nocache', '_lists'):
        base = base[:-len(suffix)] if base.endswith(suffix) else base
    if base == 'gcn34':
        import gcn_ref
        nv.set_backend_for_testing(gcn_ref.GcnAbiEmulator())
    elif base == 'squeezenet':
        import squeezenet_ref
        nv.set_backend_for_testing(squeezenet_ref.EluAbiEmulator())
    elif case.endswith('_lists'):
        from oracle import abi_emulator
        import fake_plans
        fake_plans.on_emulator(abi_emulator.AbiEmulator())
    else:
        from oracle import abi_emulator
        nv.set_backend_for_testing(abi_emulator.AbiEmulator())
    # finalize fused or not: the environment for a checkout whose Stage reads it per instance, the class attributes otherwise
    fuse = not case.endswith('_nofuse')
    os.environ['SEGNB_FUSE_FINALIZE'] = '1' if fuse else '0'
    E.Stage.fuse_finalize = NET.Tape.fuse_finalize = fuse
    E.Stage.recompute_dz_min_mb = 1e-6 if case.endswith('_src') else 0.0
    E.Stage.head_dz_recompute = not case.endswith('_headdz')
    E.UpCatConvOp.segment_wgrad, E.UpCatConvOp.segment_fwd = base.endswith('_segw'), base.endswith('_segf')
    if case == 'abn':
        return trace_abn()
    torch.manual_seed(11)
    model, x, y, dtype = make(base + ('_drop' if case.endswith('_drop') else ''), case.endswith('_nocache'))
    model.set_compute_dtype(dtype)
    if case.endswith('_eval'):
        model.eval()
        with torch.no_grad():
            model(x)
        return
    model.train()
    torch.manual_seed(13)            # (the Dropout2d multipliers: only the call text is compared, but keep it repeatable)
    for k in range(3 if case.endswith('_lists') else 1):
        if case.endswith('_lists'):
            OUT.append('--- step %d' % k)
            model.zero_grad()
            if k == 0 and not base.startswith('zf_'):
                # (the list key is only defined on a GPU: force one)
                model._plan_key = lambda x, need_grad, grads_alias: ('forced', tuple(x.shape), need_grad)
        loss = BCEWithLogitsLossAndSmoothJaccard()(model(x), y)
        if case.endswith('_lists') and k == 0 and base.startswith('zf_'):
            # (the engine exists behind the first forward, which therefore runs eagerly; its backward records)
            model._engine._cplan_key = lambda kind, *a: ('forced', kind) + tuple(str(v) for v in a[:5])
        (x.shape[0] * loss).backward()


if __name__ == '__main__':
    lines = OUT
    install(lines)
    for case in (CASES if sys.argv[1] == 'all' else sys.argv[1:2]):
        del starts[:], keep[:], lines[:]
        spans.clear()
        ordinals.clear()
        trace(case)
        print('=== %s: %d calls' % (case, sum(1 for l in lines if not l.startswith('PackTable'))))
        print('\n'.join(lines))
