"""CPU-only checks of the multi-class losses (FocalLossMulti, JaccardLossMulti, FocalAndJaccardLossMulti,
NLLLAndJaccardLossMulti; csrc/mc_loss.hip behind include/segnb_mc_loss.h):

  * the float64 restatement (tests/mc_loss_ref.py) against the reference's own values (tests/golden/losses_multi.npz);
  * lib.losses -> segnb.mcloss -> the C ABI, served by the restatement's emulator, against the same fixture;
  * the constructor surface and defaults of the reference;
  * the second ABI triple: include/segnb_mc_loss.h == the exports == segnb._native.MC_SIGNATURES | MC_PLAIN == the emulator;
  * world 2 (gloo): the all-reduced sums and the global pixel count give the single-process loss and gradient.
"""
import ctypes
import inspect
import json
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import mc_loss_ref as R
from segnb import _native as nv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'losses_multi.npz')


def _cases():
    z = np.load(GOLDEN)
    out = []
    for i in range(int(z['n_cases'])):
        cfg = json.loads(str(z['%d_cfg' % i]))
        out.append((i, cfg, torch.from_numpy(z['%d_x' % i]), torch.from_numpy(z['%d_t' % i]), torch.from_numpy(z['%d_up' % i]),
                    torch.from_numpy(z['%d_loss' % i]), torch.from_numpy(z['%d_grad' % i])))
    return out


CASES = _cases()


def make_module(cfg):
    """the lib.losses instance of a fixture case (the overlay's classes, the reference's constructor arguments)"""
    from lib import losses
    kw = dict(cfg['kw'])
    if kw.get('weight') is not None:
        kw['weight'] = torch.tensor(kw['weight'], dtype=torch.float32)
    if kw.get('class_weights') is not None:
        kw['class_weights'] = np.array(kw['class_weights'], dtype=np.float64)
    return getattr(losses, cfg['cls'])(**kw)


def check_case(loss, grad, ref_loss, ref_grad):
    """the binary family's tolerances (tests/test_hip_ops.py): loss 1e-5 relative, gradient rtol 1e-4 / atol 2e-6 max"""
    loss, grad = loss.double().cpu(), grad.double().cpu()
    ref_loss, ref_grad = ref_loss.double(), ref_grad.double()
    assert torch.allclose(loss, ref_loss, rtol=1e-5, atol=1e-7), (loss, ref_loss)
    assert torch.allclose(grad, ref_grad, rtol=1e-4, atol=2e-6 * float(ref_grad.abs().max()) + 1e-12), \
        float((grad - ref_grad).abs().max())


def test_fixture_covers_the_issue_cases():
    kinds = set()
    for _, cfg, x, t, up, loss, grad in CASES:
        kw = cfg['kw']
        C = x.shape[1]
        kinds.add(('C', C))
        kinds.add((cfg['cls'], kw.get('from_logits'), kw.get('size_average'), kw.get('gamma'), kw.get('reduce')))
        if (t == kw['ignore_index']).any():
            kinds.add('ignored')
    assert {('C', 1), ('C', 2), ('C', 5), ('C', 12), 'ignored'} <= kinds
    gammas = {k[3] for k in kinds if isinstance(k, tuple) and k[0] == 'FocalLossMulti'}
    assert {0, 1.5, 2, 3} <= gammas
    assert ('JaccardLossMulti', False, None, None, False) in kinds


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%d-%s-C%d' % (c[0], c[1]['cls'], c[2].shape[1]))
def test_restatement_matches_the_reference(case):
    i, cfg, x, t, up, ref_loss, ref_grad = case
    mod = make_module(cfg)
    c, nw, jw = R.cfg_of(mod)
    loss, _, dx = R.loss_and_grad(x, t, c, nw, jw, gout=up.reshape(-1) if up.dim() else None)
    check_case(loss, dx, ref_loss, ref_grad)


@pytest.fixture
def emulated():
    nv.set_backend_for_testing(R.McAbiEmulator())
    yield
    nv.set_backend_for_testing(None)


@pytest.mark.parametrize('one_launch', [True, False])
def test_lib_losses_through_the_abi_on_the_emulator(emulated, one_launch, monkeypatch):
    from segnb import mcloss
    monkeypatch.setattr(mcloss, '_ONE_LAUNCH', one_launch)
    for i, cfg, x, t, up, ref_loss, ref_grad in CASES:
        xr = x.clone().requires_grad_(True)
        loss = make_module(cfg)(xr, t)
        (loss * up).sum().backward()
        check_case(loss.detach(), xr.grad, ref_loss, ref_grad)


def test_imports_through_the_overlay():
    from lib.losses import FocalLossMulti, JaccardLossMulti, FocalAndJaccardLossMulti, NLLLAndJaccardLossMulti  # noqa: F401
    from lib import losses
    assert 'out of scope' not in losses.__doc__


def test_constructor_surface_and_defaults():
    from lib import losses
    want = {
        'FocalLossMulti': {'gamma': 2, 'size_average': True, 'reduce': True, 'ignore_index': -100, 'from_logits': False},
        'JaccardLossMulti': {'ignore_index': -100, 'from_logits': False, 'weight': None, 'reduce': True},
        'FocalAndJaccardLossMulti': {'jaccard_weight': 1, 'class_weights': None, 'ignore_index': -1},
        'NLLLAndJaccardLossMulti': {'jaccard_weight': 1, 'class_weights': None, 'ignore_index': -1},
    }
    for name, defaults in want.items():
        sig = inspect.signature(getattr(losses, name).__init__)
        got = {k: v.default for k, v in sig.parameters.items() if k != 'self'}
        assert got == defaults, (name, got)
    f = losses.FocalLossMulti(gamma=3, size_average=False, reduce=False, ignore_index=7, from_logits=True)
    assert (f.gamma, f.size_average, f.reduce, f.ignore_index, f.from_logits) == (3, False, False, 7, True)
    j = losses.JaccardLossMulti(weight=torch.tensor([1.0, 3.0]), reduce=False)
    assert torch.allclose(j.class_weights, torch.tensor([0.25, 0.75])) and j.reduce is False
    fj = losses.FocalAndJaccardLossMulti(jaccard_weight=2, class_weights=np.array([1.0, 1.0, 2.0]))
    assert fj.focal_loss.from_logits and fj.jaccard_loss.from_logits and fj.focal_loss.ignore_index == -1
    assert torch.allclose(fj.jaccard_loss.class_weights, torch.tensor([0.25, 0.25, 0.5]))
    nj = losses.NLLLAndJaccardLossMulti(class_weights=np.array([2.0, 1.0]))
    assert isinstance(nj.nll_loss, torch.nn.NLLLoss) and nj.nll_loss.ignore_index == -1
    assert torch.equal(nj.nll_loss.weight, torch.tensor([2.0, 1.0]))
    # get_loss keeps its keys: the reference's factory has no multi-class key
    import torch_train
    with pytest.raises(Exception):
        torch_train.get_loss('focal_multi')


def _declared_mc():
    hdr = open(os.path.join(ROOT, 'include', 'segnb_mc_loss.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    return set(re.findall(r'\b(segnb_\w+)\s*\(', hdr))


def test_mc_abi_triple():
    names = _declared_mc()
    assert names == {'segnb_mc_loss_work_doubles', 'segnb_mc_loss_reduce', 'segnb_mc_loss_finalize',
                     'segnb_mc_loss_reduce_finalize', 'segnb_mc_loss_bwd'}
    assert set(nv.MC_SIGNATURES) | set(nv.MC_PLAIN) == names
    assert not (names & (set(nv.SIGNATURES) | set(nv.PLAIN)))
    emu = R.McAbiEmulator()
    assert all(hasattr(emu, n) for n in names)
    assert [m for m in dir(emu) if m.startswith('segnb_mc_')] == sorted(names)


def test_library_exports_the_mc_entry_points():
    if not os.path.exists(nv.LIB_PATH):
        pytest.skip('libsegnb_hip.so not built (run __graft_entry__.build())')
    lib = ctypes.CDLL(nv.LIB_PATH)
    missing = [n for n in sorted(_declared_mc()) if not hasattr(lib, n)]
    assert not missing
    fn = lib.segnb_mc_loss_work_doubles
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int]
    assert fn(12) == R.McAbiEmulator().segnb_mc_loss_work_doubles(12) and fn(0) == 0 and fn(257) == 0


def test_spec_struct_layout():
    # include/segnb_mc_loss.h: int, int, long long, 5 floats, 3 ints, 2 pointers
    assert ctypes.sizeof(nv.McLossSpec) == 64
    assert nv.McLossSpec.nll_weight.offset == 48 and nv.McLossSpec.jac_weight.offset == 56


# ---------------------------------------------------------------------------------------------------------------------- world 2

def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, out_dir):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, 'segmentation-networks-benchmark_amd'), root, os.path.join(root, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    import torch.distributed as td
    import mc_loss_ref as Rw
    from segnb import _native as nvw
    from segnb import seglosses

    class CountingEmulator(Rw.McAbiEmulator):
        """counts the launches: a data-parallel job must take the two-launch form"""
        calls = []

        def segnb_mc_loss_reduce(self, *a):
            self.calls.append('reduce')
            return super().segnb_mc_loss_reduce(*a)

        def segnb_mc_loss_reduce_finalize(self, *a):
            self.calls.append('reduce_finalize')
            return super().segnb_mc_loss_reduce_finalize(*a)

    nvw.set_backend_for_testing(CountingEmulator())
    td.init_process_group('gloo', rank=rank, world_size=world)
    seglosses.DataParallelHooks.sums_allreduce = lambda s: td.all_reduce(s, op=td.ReduceOp.SUM)
    seglosses.DataParallelHooks.grad_scale = float(world)
    from lib.losses import FocalAndJaccardLossMulti, NLLLAndJaccardLossMulti
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 5, 6, 7, generator=g)
    t = torch.randint(0, 5, (4, 6, 7), generator=g)
    t[torch.rand(4, 6, 7, generator=g) < 0.2] = -1
    t[0, 0, 0] = 9                                       # a bad label: counted over both ranks
    lo, hi = rank * 2, rank * 2 + 2
    res = {}
    for name, mod in (('fj', FocalAndJaccardLossMulti(jaccard_weight=0.5, class_weights=np.arange(1.0, 6.0))),
                      ('nj', NLLLAndJaccardLossMulti(jaccard_weight=2, class_weights=np.arange(1.0, 6.0)))):
        xr = x[lo:hi].clone().requires_grad_(True)
        loss = mod(xr, t[lo:hi])
        from segnb.mcloss import mc_loss
        fin = mc_loss.last_fin.clone()
        loss.backward()
        res[name] = (float(loss), xr.grad.clone(), fin)
    torch.save({'res': res, 'calls': list(CountingEmulator.calls)}, os.path.join(out_dir, 'rank%d.pt' % rank))
    td.destroy_process_group()


def test_two_rank_sums_give_the_single_process_loss(tmp_path):
    port = _free_port()
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 5, 6, 7, generator=g)
    t = torch.randint(0, 5, (4, 6, 7), generator=g)
    t[torch.rand(4, 6, 7, generator=g) < 0.2] = -1
    t[0, 0, 0] = 9
    from lib.losses import FocalAndJaccardLossMulti, NLLLAndJaccardLossMulti
    mods = {'fj': FocalAndJaccardLossMulti(jaccard_weight=0.5, class_weights=np.arange(1.0, 6.0)),
            'nj': NLLLAndJaccardLossMulti(jaccard_weight=2, class_weights=np.arange(1.0, 6.0))}
    outs = [torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r)) for r in range(2)]
    for o in outs:
        assert 'reduce_finalize' not in o['calls'] and o['calls'].count('reduce') == 2
    for name, mod in mods.items():
        c, nw, jw = R.cfg_of(mod)
        loss, fin, dx = R.loss_and_grad(x, t, c, nw, jw)
        for r, o in enumerate(outs):
            l_r, g_r, fin_r = o['res'][name]
            assert abs(l_r - float(loss)) <= 1e-6 * abs(float(loss)), (name, r, l_r, float(loss))
            assert float(fin_r[4]) == x.shape[0] * 6 * 7 and float(fin_r[5]) == 1.0   # GLOBAL pixel and bad-label counts
            # the backward seed times the world size (seglosses.DataParallelHooks.grad_scale)
            want = 2.0 * dx[r * 2:r * 2 + 2]
            assert torch.allclose(g_r.double(), want, rtol=1e-4, atol=2e-6 * float(want.abs().max())), name
