"""CPU-only checks of GCN34 (lib.models.gcn over segnb.gcn and csrc/gcn.hip behind include/segnb_gcn.h):

  * the float64 restatement (tests/gcn_ref.py) against the reference's own values (tests/golden/gcn34_small.npz: K = 1,
    K = 3 with a dot-product loss, and a 64 -> 80 final resize);
  * GCN34 through the C ABI, served by the restatement's emulator, against the same fixture;
  * the state_dict layout of the reference, the driver's get_model('gcn34'), the input checks;
  * the third ABI triple: include/segnb_gcn.h == the exports == segnb._native.GCN_SIGNATURES | GCN_PLAIN == the emulator.
"""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

import gcn_ref as R
import model_checks as mc
from segnb import _native as nv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'gcn34_small.npz')
CASES = {'k1': (1, 64), 'k3': (3, 96), 'rs': (1, 80)}         # prefix -> (num_classes, input_size)


class Case(object):
    """One case of the fixture, read like a single-case npz (the keys without the prefix; fp16-stored inputs as fp32)."""

    def __init__(self, z, prefix):
        self.z, self.prefix = z, prefix + '_'
        self.files = [k[len(self.prefix):] for k in z.files if k.startswith(self.prefix)]

    def __getitem__(self, k):
        v = self.z[self.prefix + k]
        return v.astype(np.float32) if v.dtype == np.float16 else v


def load_case(prefix):
    return Case(np.load(GOLDEN), prefix)


def make_gcn(prefix, golden):
    """the product GCN34 of a fixture case with the seeded fill (state_dict keys and numels asserted by _load_seeded)"""
    from lib.models.gcn import GCN34
    K, size = CASES[prefix]
    m = GCN34(num_classes=K, input_size=size, pretrained=False)
    for g in (m.gcm1, m.gcm2, m.gcm3, m.gcm4):
        g.pre_drop.p = 0.0
    return mc._load_seeded(m, golden)


def check_dot_case(model, golden, device, dtype='f32'):
    """K = 3 case: loss = (logits * G).sum(), gradients against the fixture (check_product_golden's fp32 tolerances)"""
    x, G = torch.from_numpy(golden['x']), torch.from_numpy(golden['G'])
    model.set_compute_dtype(dtype)
    model.to(device)
    model.eval()
    with torch.no_grad():
        ev = model(x.to(device))
    scale = float(np.abs(golden['eval_logits']).max())
    assert float(np.abs(ev.cpu().numpy() - golden['eval_logits']).max()) <= 2e-4 * scale
    model.train()
    out = model(x.to(device))
    assert out.shape == G.shape
    loss = (out * G.to(device)).sum()
    loss.backward()
    scale = float(np.abs(golden['train_logits']).max())
    assert float(np.abs(out.detach().cpu().numpy() - golden['train_logits']).max()) <= 2e-4 * scale
    ref = float(golden['loss_dot'])
    assert abs(loss.item() - ref) <= 1e-4 * abs(ref), (loss.item(), ref)
    mc._check_grads_golden({n: p.grad for n, p in model.named_parameters()}, golden, 1e-2, 5e-2)


@pytest.fixture
def emulated():
    nv.set_backend_for_testing(R.GcnAbiEmulator())
    yield
    nv.set_backend_for_testing(None)


@pytest.mark.parametrize('prefix', sorted(CASES))
def test_restatement_matches_the_reference(prefix):
    from oracle import losses_ref
    g = load_case(prefix)
    K, size = CASES[prefix]
    m = make_gcn(prefix, g)
    sd = {k: v.detach().clone().double() if v.is_floating_point() else v.clone() for k, v in m.state_dict().items()}
    pnames = [n for n, _ in m.named_parameters()]
    x = torch.from_numpy(g['x']).double()
    with torch.no_grad():
        ev = R.forward({k: v.clone() for k, v in sd.items()}, x, size, train=False)
    np.testing.assert_allclose(ev.numpy(), g['eval_logits'], rtol=1e-4, atol=2e-5 * float(np.abs(g['eval_logits']).max()))
    leaves = {k: (v.clone().requires_grad_(True) if k in pnames else v.clone()) for k, v in sd.items()}
    logits = R.forward(leaves, x, size, train=True)
    np.testing.assert_allclose(logits.detach().numpy(), g['train_logits'], rtol=1e-4,
                               atol=2e-5 * float(np.abs(g['train_logits']).max()))
    if prefix == 'k3':
        loss = (logits * torch.from_numpy(g['G']).double()).sum()
        assert abs(loss.item() - float(g['loss_dot'])) <= 1e-5 * abs(float(g['loss_dot']))
        loss.backward()
    else:
        loss = losses_ref.bce_jaccard(logits, torch.from_numpy(g['y']))
        assert abs(loss.item() - float(g['loss_bce_jaccard'])) < 1e-5
        (x.shape[0] * loss).backward()
    mc._check_grads_golden({n: leaves[n].grad for n in pnames}, g, 1e-3, 2e-3)


@pytest.mark.parametrize('prefix', sorted(CASES))
def test_gcn34_through_the_abi_on_the_emulator(emulated, prefix):
    g = load_case(prefix)
    m = make_gcn(prefix, g)
    if prefix == 'k3':
        check_dot_case(m, g, 'cpu')
    else:
        mc.check_product_golden(m, g, 'cpu')


def test_state_dict_layout_is_the_reference():
    for prefix in CASES:
        g = load_case(prefix)
        m = make_gcn(prefix, g)                        # (asserts keys and numels)
        keys = list(m.state_dict())
        assert keys[0] == 'layer0.0.weight' and 'layer1.1.0.conv1.weight' in keys and 'gcm4.conv_r2.bias' in keys
        assert keys[-1] == 'brm9.conv2.bias'


def test_driver_get_model():
    import torch_train
    from lib.models.gcn import GCN34
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = torch_train.get_model('gcn34', 64)
    assert isinstance(m, GCN34) and m.num_classes == 1 and m.input_size == 64
    assert m.gcm1.conv_l1.weight.shape == (1, 512, 7, 1) and m.gcm4.conv_r1.weight.shape == (1, 64, 1, 7)
    assert float(m.brm3.conv1.bias.abs().max()) == 0.0           # the reference's initialize_weights: zero biases
    with pytest.raises(ValueError):
        torch_train.get_model('gcn', 64)                          # GCN152: not built


def test_input_checks(emulated):
    from lib.models.gcn import GCN34
    m = GCN34(num_classes=2, input_size=(64, 96), pretrained=False)
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 48, 64))
    with pytest.raises(ValueError):
        GCN34(num_classes=33, input_size=64, pretrained=False)
    m.eval()
    with torch.no_grad():
        out = m(torch.randn(1, 3, 64, 64))
    assert out.shape == (1, 2, 64, 96)


def _declared_gcn():
    hdr = open(os.path.join(ROOT, 'include', 'segnb_gcn.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    return set(re.findall(r'\b(segnb_\w+)\s*\(', hdr))


def test_gcn_abi_triple():
    names = _declared_gcn()
    assert names == {'segnb_gcn_ok', 'segnb_gcm_fwd', 'segnb_gcm_bwd', 'segnb_brm_fwd', 'segnb_brm_bwd',
                     'segnb_resize_bilinear_ac_fwd', 'segnb_resize_bilinear_ac_bwd'}
    assert set(nv.GCN_SIGNATURES) | set(nv.GCN_PLAIN) == names
    assert not (names & (set(nv.SIGNATURES) | set(nv.PLAIN) | set(nv.MC_SIGNATURES) | set(nv.MC_PLAIN)))
    emu = R.GcnAbiEmulator()
    assert all(hasattr(emu, n) for n in names)
    gcn_methods = {m for m in dir(emu) if m.startswith(('segnb_gcm_', 'segnb_brm_', 'segnb_gcn_', 'segnb_resize_'))}
    assert gcn_methods == names
    # argument counts: header == ctypes table
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'segnb_gcn.h')).read(), flags=re.S)
    for name, args in re.findall(r'\bint\s+(segnb_\w+)\s*\(([^)]*)\)', hdr):
        n = len([a for a in args.split(',') if a.strip()])
        argtypes = nv.GCN_SIGNATURES[name] if name in nv.GCN_SIGNATURES else nv.GCN_PLAIN[name][1]
        assert len(argtypes) == n, (name, len(argtypes), n)


def test_library_exports_the_gcn_entry_points():
    if not os.path.exists(nv.LIB_PATH):
        pytest.skip('libsegnb_hip.so not built (run __graft_entry__.build())')
    lib = ctypes.CDLL(nv.LIB_PATH)
    missing = [n for n in sorted(_declared_gcn()) if not hasattr(lib, n)]
    assert not missing
    fn = lib.segnb_gcn_ok
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 5
    emu = R.GcnAbiEmulator()
    for args in [(64, 1, 16, 128, 128), (512, 32, 16, 16, 16), (2048, 32, 1, 8, 8), (0, 3, 2, 80, 80), (60, 1, 1, 8, 8),
                 (64, 0, 1, 8, 8), (64, 33, 1, 8, 8), (4096, 1, 1, 8, 8), (8, 32, 1 << 10, 1 << 10, 1 << 6)]:
        assert fn(*args) == emu.segnb_gcn_ok(*args), args
