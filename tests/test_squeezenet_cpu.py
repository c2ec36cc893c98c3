"""CPU-only checks of SqueezeNet (lib.models.squeezenet over segnb.net.elu and csrc/elu.hip behind include/segnb_elu.h):

  * the float64 restatement (tests/squeezenet_ref.py) against the reference's own values (tests/golden/squeezenet_small.npz:
    2x3x32x32 with bce_jaccard, 1x3x24x40 with a dot-product loss);
  * SqueezeNet through the C ABI, served by the restatement's emulator, against the same fixture;
  * the state_dict layout of the reference, the driver's get_model('squeezenet'), the input checks;
  * the ELU pass takes over the backward of the convolutions in front of it (Act.g_is_dz), and falls back when it may not;
  * the fourth ABI triple: include/segnb_elu.h == the exports == segnb._native.ELU_SIGNATURES | ELU_PLAIN == the emulator.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import model_checks as mc
import squeezenet_ref as R
from segnb import _native as nv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'squeezenet_small.npz')
HEADER = os.path.join(ROOT, 'include', 'segnb_elu.h')
CASES = ('sq', 'ns')
ELU_NAMES = {'segnb_elu_ok', 'segnb_elu_fwd', 'segnb_elu_bwd'}


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


def make_squeezenet(golden):
    """the product SqueezeNet with the fixture's seeded fill (state_dict keys and numels asserted by _load_seeded)"""
    from lib.models.squeezenet import SqueezeNet
    return mc._load_seeded(SqueezeNet(in_channels=3, num_classes=1), golden)


def check_dot_case(model, golden, device, dtype='f32'):
    """ns_ case: loss = (logits * G).sum(), gradients against the fixture (check_product_golden's fp32 tolerances)"""
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
    nv.set_backend_for_testing(R.EluAbiEmulator())
    yield
    nv.set_backend_for_testing(None)


@pytest.mark.parametrize('prefix', CASES)
def test_restatement_matches_the_reference(prefix):
    from oracle import losses_ref
    g = load_case(prefix)
    m = make_squeezenet(g)
    sd = {k: v.detach().clone().double() for k, v in m.state_dict().items()}
    pnames = [n for n, _ in m.named_parameters()]
    x = torch.from_numpy(g['x']).double()
    with torch.no_grad():
        ev = R.forward(sd, x)
    np.testing.assert_allclose(ev.numpy(), g['eval_logits'], rtol=1e-4, atol=2e-5 * float(np.abs(g['eval_logits']).max()))
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    logits = R.forward(leaves, x)
    np.testing.assert_allclose(logits.detach().numpy(), g['train_logits'], rtol=1e-4,
                               atol=2e-5 * float(np.abs(g['train_logits']).max()))
    if prefix == 'ns':
        loss = (logits * torch.from_numpy(g['G']).double()).sum()
        assert abs(loss.item() - float(g['loss_dot'])) <= 1e-5 * abs(float(g['loss_dot']))
        loss.backward()
    else:
        loss = losses_ref.bce_jaccard(logits, torch.from_numpy(g['y']))
        assert abs(loss.item() - float(g['loss_bce_jaccard'])) < 1e-5
        (x.shape[0] * loss).backward()
    mc._check_grads_golden({n: leaves[n].grad for n in pnames}, g, 1e-3, 2e-3)


@pytest.mark.parametrize('prefix', CASES)
def test_squeezenet_through_the_abi_on_the_emulator(emulated, prefix):
    g = load_case(prefix)
    m = make_squeezenet(g)
    if prefix == 'ns':
        check_dot_case(m, g, 'cpu')
    else:
        mc.check_product_golden(m, g, 'cpu')


def test_state_dict_layout_is_the_reference():
    for prefix in CASES:
        g = load_case(prefix)
        m = make_squeezenet(g)                        # (asserts key order and numels)
        keys = list(m.state_dict())
        assert len(keys) == 104
        assert keys[0] == 'conv1.weight' and keys[-1] == 'dconv1.bias'
        for k in ('fire2.squeeze.weight', 'conv10.0.weight', 'dconv10.0.bias', 'dfire2.squeeze.bias', 'dfire9.expand3x3.weight'):
            assert k in keys, k
        assert sum(p.numel() for p in m.parameters()) == 7549057


def test_default_initialisation_is_torchs():
    """the reference sets no initialisation: nn.Conv2d's own (kaiming_uniform(a = sqrt(5)): |w| <= 1 / sqrt(fan_in))"""
    from lib.models.squeezenet import SqueezeNet
    torch.manual_seed(3)
    m = SqueezeNet()
    for conv in (m.conv1, m.fire4.expand3x3, m.conv10[0], m.dconv1):
        bound = 1.0 / np.sqrt(conv.in_channels * conv.kernel_size[0] * conv.kernel_size[1])
        assert float(conv.weight.abs().max()) <= bound and float(conv.weight.abs().max()) > 0.5 * bound
        assert float(conv.bias.abs().max()) <= bound and float(conv.bias.abs().max()) > 0.0


def test_driver_get_model():
    import torch_train
    from lib.models.squeezenet import SqueezeNet
    m = torch_train.get_model('squeezenet')
    assert isinstance(m, SqueezeNet) and m.num_classes == 1
    assert m.conv1.weight.shape == (96, 3, 3, 3) and m.dconv1.weight.shape == (1, 96, 1, 1)
    assert m.lazy_add is True


def test_input_checks(emulated):
    from lib.models.squeezenet import Fire, SqueezeNet
    m = SqueezeNet()
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 20, 32))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 4, 32, 32))
    with pytest.raises(ValueError):
        SqueezeNet(in_channels=4)
    with pytest.raises(ValueError):
        SqueezeNet(num_classes=33)
    with pytest.raises(RuntimeError):
        Fire(96, 16, 64, 64)(torch.zeros(1, 96, 8, 8))
    m.eval()
    with torch.no_grad():
        out = m(torch.randn(1, 3, 8, 16))
    assert out.shape == (1, 1, 8, 16)


class _Recording(R.EluAbiEmulator):
    """the emulator, remembering the sums arguments of segnb_elu_bwd"""

    def __init__(self):
        self.elu_sums = []

    def segnb_elu_bwd(self, *a):
        self.elu_sums.append((bool(a[15]), a[16], bool(a[17])))
        return R.EluAbiEmulator.segnb_elu_bwd(self, *a)


def _count_calls(monkeypatch):
    """-> the list the product's ABI calls (segnb._native.call) are appended to, by name"""
    calls, orig = [], nv.call

    def call(name, *a):
        calls.append(name)
        return orig(name, *a)
    monkeypatch.setattr(nv, 'call', call)
    return calls


def test_elu_writes_the_gradient_of_the_convolutions_in_front_of_it(monkeypatch):
    """SqueezeNet's 34 ELU passes: every one serves its producers (18 single convolutions: the 16 squeezes, conv10, dconv10; 16
    concat pairs over two tables) -- no convolution but conv1 runs a reduction pass of its own."""
    emu = _Recording()
    calls = _count_calls(monkeypatch)
    nv.set_backend_for_testing(emu)
    try:
        g = load_case('sq')
        m = make_squeezenet(g).set_compute_dtype('f32').train()
        x = torch.from_numpy(g['x'])
        m(x).sum().backward()
    finally:
        nv.set_backend_for_testing(None)
    assert calls.count('segnb_elu_fwd') == 34 and calls.count('segnb_elu_bwd') == 34
    assert len(emu.elu_sums) == 34 and all(s[0] for s in emu.elu_sums)
    assert sum(1 for s in emu.elu_sums if s[2]) == 16                     # the 8 Fire and 8 DFire expand pairs
    # conv1 has two consumers and no ELU: its own pass, over two sources (the pooling's and the skip add's gradient)
    assert calls.count('segnb_bn_act_bwd_reduce_add') == 1 and calls.count('segnb_bn_act_bwd_reduce') == 0
    # the only add passes: the two upsampled sums that feed two expand convolutions (dfire8, dfire4) -- their summed gradient is
    # also the skip operand's, so it has to exist; every other two-consumer tensor hands both gradients to its ELU pass
    assert calls.count('segnb_add') == 2


# ---- a small net around one ELU: the producer protocol, its fallback and the upsample-add at the operator level ------------
def make_probe_net(mode):
    """conv 1x1 -> elu -> conv 1x1 -> head ('chain'); the same with the raw convolution output read a second time, by an add
    ('second_consumer': elu must contribute a plain gradient); 'upskip': the first convolution's output is pooled, convolved,
    and elu(up_skip=that output) adds the upsampled activation back.  The views of the ELU are kept in .probe."""
    from torch import nn
    from segnb import convplan as cp
    from segnb.net import HipNet, add, conv_unit, elu, head_1x1, maxpool

    class ProbeNet(HipNet):
        def __init__(self):
            super(ProbeNet, self).__init__()
            self.c1 = nn.Conv2d(3, 96, 1)
            self.c3 = nn.Conv2d(96, 96, 1)
            self.c2 = nn.Conv2d(96, 16, 1)
            self.head = nn.Conv2d(16, 1, 1)
            self.probe = {}
            self._init_engine(3)

        def _build(self, tape, x, dlogits):
            def conv(t, m, tag):
                return conv_unit(tape, t, m.weight, m.bias, [(m.in_channels, cp.pad8(m.in_channels))], stride=1, pad=0,
                                 act=nv.ACT_NONE, tag=tag)
            y = conv(x, self.c1, 'c1')
            if mode == 'chain':
                s = elu(tape, y)
            elif mode == 'second_consumer':
                yv = y.v
                a = elu(tape, y, out=tape.view('probe/a', yv.N, yv.H, yv.W, yv.Cp))
                s = add(tape, a, y)
            else:
                z = conv(maxpool(tape, y, 2, 2, 0), self.c3, 'c3')
                zv = z.v
                a, s = elu(tape, z, up_skip=y, out=tape.view('probe/a', zv.N, zv.H, zv.W, zv.Cp))
                self.probe = dict(z=zv, a=a.v, up=s.v, skip=y.v)
            return head_1x1(tape, conv(s, self.c2, 'c2'), self.head.weight, self.head.bias, dlogits)

    torch.manual_seed(11)
    return ProbeNet()


def probe_reference(m, mode, x, G):
    """float64 torch: -> (logits, {parameter name: gradient of (logits * G).sum()})"""
    import torch.nn.functional as F
    ps = {n: p.detach().cpu().double().requires_grad_(True) for n, p in m.named_parameters()}

    def conv(t, k):
        return F.conv2d(t, ps[k + '.weight'], ps[k + '.bias'])
    y = conv(x.double(), 'c1')
    if mode == 'chain':
        s = F.elu(y)
    elif mode == 'second_consumer':
        s = F.elu(y) + y
    else:
        s = R.up2(F.elu(conv(F.max_pool2d(y, 2, 2), 'c3'))) + y
    lo = conv(conv(s, 'c2'), 'head')
    (lo * G.double()).sum().backward()
    return lo.detach(), {n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in ps.items()}


def check_probe_net(mode, device, monkeypatch, dtype='f32', rtol=1e-4, check_grads=True):
    """one step of the probe net against float64; -> (net, names of the ABI calls of the step).  rtol: of the logits' scale, and
    of each gradient tensor's L2 norm.  check_grads False: the logits alone -- in bf16 the pooled mode routes gradients by the
    maxima of bf16-rounded values, which tie where float64's do not (a discrete difference, not a rounding error)."""
    m = make_probe_net(mode).set_compute_dtype(dtype).to(device).train()
    g = torch.Generator().manual_seed(5)
    x, G = torch.randn((2, 3, 12, 20), generator=g), torch.randn((2, 1, 12, 20), generator=g)
    ref_lo, ref_g = probe_reference(m, mode, x, G)
    calls = _count_calls(monkeypatch)
    out = m(x.to(device))
    (out * G.to(device)).sum().backward()
    scale = float(ref_lo.abs().max())
    assert float((out.detach().cpu().double() - ref_lo).abs().max()) <= rtol * scale
    for n, p in m.named_parameters():
        if not check_grads or (mode != 'upskip' and n.startswith('c3')):
            continue
        err = float((p.grad.detach().cpu().double() - ref_g[n]).norm() / ref_g[n].norm())
        assert err <= rtol, (mode, n, err)
    return m, calls


def test_probe_chain_elu_serves_the_first_convolution(monkeypatch, emulated):
    m, calls = check_probe_net('chain', 'cpu', monkeypatch)
    assert calls.count('segnb_elu_bwd') == 1
    assert calls.count('segnb_bn_act_bwd_reduce') == 0 and calls.count('segnb_bn_act_bwd_reduce_add') == 0


def test_probe_second_consumer_falls_back_to_a_plain_gradient(monkeypatch, emulated):
    m, calls = check_probe_net('second_consumer', 'cpu', monkeypatch)
    assert calls.count('segnb_elu_bwd') == 1
    assert calls.count('segnb_bn_act_bwd_reduce') == 1               # the first convolution sums its own gradient


def test_probe_upskip_gradients(monkeypatch, emulated):
    check_probe_net('upskip', 'cpu', monkeypatch)


def test_elu_in_place_refuses_a_tensor_with_another_reader(emulated):
    """the probe net's second-consumer mode WITHOUT out=: the add registered after the ELU would read activated values"""
    from torch import nn
    from segnb import convplan as cp
    from segnb.net import HipNet, add, conv_unit, elu, head_1x1, maxpool

    class Bad(HipNet):
        def __init__(self, pool_first):
            super(Bad, self).__init__()
            self.c1, self.head, self.pool_first = nn.Conv2d(3, 8, 1), nn.Conv2d(8, 1, 1), pool_first
            self._init_engine(3)

        def _build(self, tape, x, dlogits):
            y = conv_unit(tape, x, self.c1.weight, self.c1.bias, [(3, cp.pad8(3))], stride=1, pad=0, act=nv.ACT_NONE)
            if self.pool_first:
                maxpool(tape, y, 2, 2, 0)
            s = add(tape, elu(tape, y), y)
            return head_1x1(tape, s, self.head.weight, self.head.bias, dlogits)

    with pytest.raises(ValueError):                   # a reader registered before the pass: refused in the forward
        Bad(True).train()(torch.randn(1, 3, 8, 8))
    out = Bad(False).train()(torch.randn(1, 3, 8, 8))
    with pytest.raises(RuntimeError):                 # one registered after it: refused in the backward
        out.sum().backward()


def test_squeezenet_at_its_smallest_maps(emulated, monkeypatch):
    """16 x 16 input: 2 x 2 maps at the bottom (fire9 .. dfire9, 512 -> 1024 -> 512 at 1 x 1 kernels, 3 x 3 at 64 -> 256 and
    512 -> 256).  Every convolution stays on its fused-epilogue path -- all 34 ELU passes serve their producers, as at 32 x 32 --
    and the step matches the float64 restatement."""
    from oracle import fill
    from lib.models.squeezenet import SqueezeNet
    m = SqueezeNet()
    m.load_state_dict(fill.seeded_state(m.state_dict(), 7))
    m.set_compute_dtype('f32').train()
    g = torch.Generator().manual_seed(3)
    x, G = torch.randn((1, 3, 16, 16), generator=g), torch.randn((1, 1, 16, 16), generator=g)
    sd = {k: v.detach().clone().double().requires_grad_(True) for k, v in m.state_dict().items()}
    ref = R.forward(sd, x.double())
    (ref * G.double()).sum().backward()
    calls = _count_calls(monkeypatch)
    out = m(x)
    (out * G).sum().backward()
    assert float((out.detach().double() - ref.detach()).abs().max()) <= 2e-4 * float(ref.detach().abs().max())
    for n, p in m.named_parameters():
        err = float((p.grad.double() - sd[n].grad).norm() / (sd[n].grad.norm() + 1e-30))
        assert err <= 1e-3, (n, err)
    assert calls.count('segnb_elu_bwd') == 34
    assert calls.count('segnb_bn_act_bwd_reduce') == 0 and calls.count('segnb_bn_act_bwd_reduce_add') == 1


def _declared():
    hdr = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return hdr, set(re.findall(r'\b(segnb_\w+)\s*\(', hdr))


def test_elu_abi_triple():
    hdr, names = _declared()
    assert names == ELU_NAMES
    assert set(nv.ELU_SIGNATURES) | set(nv.ELU_PLAIN) == names
    others = (set(nv.SIGNATURES) | set(nv.PLAIN) | set(nv.MC_SIGNATURES) | set(nv.MC_PLAIN) | set(nv.GCN_SIGNATURES)
              | set(nv.GCN_PLAIN))
    assert not (names & others)
    emu = R.EluAbiEmulator()
    assert {m for m in dir(emu) if m.startswith('segnb_elu_')} == names
    for name, args in re.findall(r'\bint\s+(segnb_\w+)\s*\(([^)]*)\)', hdr):
        n = len([a for a in args.split(',') if a.strip()])
        argtypes = nv.ELU_SIGNATURES[name] if name in nv.ELU_SIGNATURES else nv.ELU_PLAIN[name][1]
        assert len(argtypes) == n, (name, len(argtypes), n)
    # nothing outside the new files knows an ELU activation code
    assert 'ACT_ELU' not in open(os.path.join(ROOT, 'include', 'segnb_hip.h')).read()


def test_library_exports_the_elu_entry_points():
    assert os.path.exists(nv.LIB_PATH), 'libsegnb_hip.so not built (run __graft_entry__.build())'
    lib = ctypes.CDLL(nv.LIB_PATH)
    missing = [n for n in sorted(ELU_NAMES) if not hasattr(lib, n)]
    assert not missing
    fn = lib.segnb_elu_ok
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 5
    emu = R.EluAbiEmulator()
    for args in [(0, 1, 1, 1, 8), (1, 16, 512, 512, 96), (1, 2, 5, 7, 1024), (0, 16, 256, 256, 128), (1, 1, 1, 1, 1032),
                 (1, 1, 1, 1, 4), (1, 1, 1, 1, 12), (2, 1, 8, 8, 8), (0, 0, 8, 8, 8), (0, 1 << 10, 1 << 10, 1 << 7, 8),
                 (1, 32, 2048, 2048, 8)]:
        assert fn(*args) == emu.segnb_elu_ok(*args), args
    assert fn(1, 16, 512, 512, 96) == 1 and fn(0, 1, 1, 1, 1024) == 1 and fn(1, 1, 1, 1, 1032) == 0
