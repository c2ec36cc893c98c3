"""CPU-only checks of UNet, UNetABN and Afterburner (lib.models.{unet, unet_abn, afterburner} over
segnb.net.upsample_nearest2x and the two nearest-upsample launches of csrc/elementwise.hip behind include/segnb_upsample.h):

  * the restatement (tests/unet_ref.py) against the reference's own values (tests/golden/unet_small.npz, five cases): the pin;
  * the product models through the C ABI, served by the restatement's emulator, in fp32 against the same fixture with
    check_product_golden's bounds;
  * state_dict key lists and element counts of the five constructions;
  * n_filters = 12 (padded concat slices 12 -> 16, 24, 48, 96): eval and one training step against the float64 restatement;
  * the input checks, the driver's get_model('unet' | 'unet_abn'), Afterburner;
  * the operator alone: forward copy, backward scan-order sum, the no-gradient and needs_grad = False paths;
  * the fifth ABI triple: include/segnb_upsample.h == the exports == segnb._native.UP_SIGNATURES == the emulator.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import model_checks as mc
import unet_ref as R
from segnb import _native as nv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'unet_small.npz')
HEADER = os.path.join(ROOT, 'include', 'segnb_upsample.h')
CASES = tuple(R.CASES)
UP_NAMES = {'segnb_upsample_nearest2x_fwd', 'segnb_upsample_nearest2x_bwd'}


class Case(object):
    """One case of the fixture, read like a single-case npz (the keys without the prefix; fp16-stored inputs as fp32)."""

    def __init__(self, z, prefix):
        self.z, self.prefix = z, prefix + '_'
        self.files = [k[len(self.prefix):] for k in z.files if k.startswith(self.prefix)]

    def __getitem__(self, k):
        v = self.z[self.prefix + k]
        return v.astype(np.float32) if v.dtype == np.float16 else v


_Z = []


def load_case(prefix):
    if not _Z:
        _Z.append(np.load(GOLDEN))
    return Case(_Z[0], prefix)


def construct(prefix, n_filters=8):
    """the product model of a fixture case, finaldrop off as in the generator"""
    from lib.models.unet import UNet
    from lib.models.unet_abn import UNetABN
    name, kw = R.CASES[prefix]
    m = {'UNet': UNet, 'UNetABN': UNetABN}[name](n_filters=n_filters, **kw)
    m.finaldrop.p = 0.0
    return m


def make_model(prefix, golden):
    """... with the fixture's seeded fill (state_dict keys and numels asserted by _load_seeded)"""
    return mc._load_seeded(construct(prefix), golden)


@pytest.fixture
def emulated():
    nv.set_backend_for_testing(R.UpsampleAbiEmulator())
    yield
    nv.set_backend_for_testing(None)


@pytest.mark.parametrize('prefix', CASES)
def test_restatement_matches_the_reference(prefix):
    g = load_case(prefix)
    m = make_model(prefix, g)
    fwd = R.forward_for(prefix)
    mc.check_oracle_golden(lambda sd, x: fwd(sd, x, True), lambda sd, x: fwd(sd, x, False), m, g)
    # float64: the same, tighter (the fixture's own fp32 noise is all that is left)
    sd = {k: v.detach().clone().double() if v.is_floating_point() else v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ev = fwd(sd, torch.from_numpy(g['x']).double(), False)
    assert float(np.abs(ev.numpy() - g['eval_logits']).max()) <= 2e-5 * float(np.abs(g['eval_logits']).max())


@pytest.mark.parametrize('prefix', CASES)
def test_product_through_the_abi_on_the_emulator(emulated, prefix):
    g = load_case(prefix)
    mc.check_product_golden(make_model(prefix, g), g, 'cpu')


def test_state_dict_layout_is_the_reference():
    counts = {}
    for prefix in CASES:
        g = load_case(prefix)
        m = make_model(prefix, g)                     # (asserts key order and numels against the fixture)
        keys = list(m.state_dict())
        counts[prefix] = (len(keys), sum(p.numel() for p in m.parameters()))
        assert keys[0] == 'inc.conv.conv.0.weight' and keys[-1] == 'outc.conv.bias'
        if prefix == 'abn':
            for k in ('inc.conv.conv.1.running_var', 'down1.mpconv.1.conv.3.running_var', 'up1.conv.conv.2.weight'):
                assert k in keys, k
            assert not [k for k in keys if 'num_batches_tracked' in k or '.conv.4.' in k]
        else:
            for k in ('down1.mpconv.1.conv.4.running_var', 'up1.conv.conv.1.num_batches_tracked', 'up4.conv.conv.3.bias'):
                assert k in keys, k
        assert ('up1.up.weight' in keys) == (prefix == 'dc') and ('up4.up.bias' in keys) == (prefix == 'dc')
    # 18 convolutions + 18 normalisations + the classifier; the deconvolution branch adds four weight / bias pairs
    assert counts['sq'] == (18 * 2 + 18 * 5 + 2, 210801) and counts['dc'] == (counts['sq'][0] + 8, 232681)
    assert counts['abn'] == (18 * 2 + 18 * 4 + 2, 210801) and counts['g1'][1] == 210801 - 2 * 8 * 9
    # the default constructions: the reference's sizes
    from lib.models.unet import UNet, double_conv, down, inconv, outconv, up
    m = UNet()
    assert m.num_classes == 1 and m.inc.conv.conv[0].weight.shape == (32, 3, 3, 3) and m.up1.conv.conv[0].weight.shape == (128, 512, 3, 3)
    assert isinstance(m.inc, inconv) and isinstance(m.down4, down) and isinstance(m.up4, up) and isinstance(m.outc, outconv)
    assert isinstance(m.down2.mpconv[1], double_conv) and isinstance(m.up2.up, torch.nn.Upsample)
    assert UNet(upsample=False).up1.up.weight.shape == (256, 256, 2, 2)
    with pytest.raises(RuntimeError):
        m.inc(torch.zeros(1, 3, 16, 16))              # a parameter holder


@pytest.mark.parametrize('name', ['UNet', 'UNetABN'])
def test_padded_slices_at_12_filters(emulated, name):
    """n_filters = 12: the concat buffers are [12 -> 16 | 12 -> 16], [24 | 24], [48 | 48], [96 | 96] -- the level-0 slices
    carry four padding channels each, which the convolution over the concat must skip.  Eval logits and one training step
    (loss = (logits * G).sum()) against the float64 restatement.  Bounds: the logits at check_product_golden's 2e-4 of their
    scale; every gradient tensor within 1e-3 relative L2, a tenth of check_product_golden's norm bound -- fp32 rounding through
    23 layers is 1e-5 here, what costs 1e-2 is an activation flipping side, so the seeds are a condition as in the fixture: the
    restatement in fp32 must itself be within 1e-4 of float64 (asserted).  Weights 33 / batch 6 give 6e-6 for both models;
    31 / 4 has a pre-activation 3e-6 from zero on a map of scale 5.7 (four fp32 ulps) and is not used."""
    from oracle import fill
    prefix = 'abn' if name == 'UNetABN' else 'sq'
    m = construct(prefix, n_filters=12)
    m.load_state_dict(fill.seeded_state(m.state_dict(), 33))
    m.set_compute_dtype('f32')
    gen = torch.Generator().manual_seed(6)
    x, G = torch.randn((2, 3, 32, 48), generator=gen), torch.randn((2, 1, 32, 48), generator=gen)
    fwd = R.forward_for(prefix)
    pnames = [n for n, _ in m.named_parameters()]

    def sd_as(dt):
        return {k: (v.detach().clone().to(dt) if v.is_floating_point() else v.clone()) for k, v in m.state_dict().items()}

    def restated(dt):
        leaves = sd_as(dt)
        for n in pnames:
            leaves[n].requires_grad_(True)
        lo = fwd(leaves, x.to(dt), True)
        (lo * G.to(dt)).sum().backward()
        return lo, leaves
    with torch.no_grad():
        ref_ev = fwd(sd_as(torch.float64), x.double(), False)
    ref, leaves = restated(torch.float64)
    _, leaves32 = restated(torch.float32)
    gmax = max(float(leaves[n].grad.norm()) for n in pnames)
    live = [n for n in pnames if float(leaves[n].grad.norm()) >= 1e-6 * gmax]      # (not: a convolution bias in front of a normalisation)
    for n in live:
        r = leaves[n].grad
        assert float((leaves32[n].grad.double() - r).norm() / r.norm()) <= 1e-4, ('the restatement in fp32', n)
    m.eval()
    with torch.no_grad():
        ev = m(x)
    assert float((ev.double() - ref_ev).abs().max()) <= 2e-4 * float(ref_ev.abs().max())
    m.train()
    out = m(x)
    (out * G).sum().backward()
    assert float((out.detach().double() - ref.detach()).abs().max()) <= 2e-4 * float(ref.detach().abs().max())
    got = dict(m.named_parameters())
    for n in live:
        r = leaves[n].grad
        err = float((got[n].grad.double() - r).norm() / r.norm())
        assert err <= 1e-3, (n, err)


def test_input_checks_driver_and_afterburner(emulated):
    import torch_train
    from lib.models.afterburner import Afterburner
    from lib.models.unet import UNet
    from lib.models.unet_abn import UNetABN
    from lib.modules.abn import InPlaceABN
    m = construct('sq')
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 24, 40))                  # the reference would return 16 x 32 logits here
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 32, 40))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 4, 32, 32))
    with pytest.raises(ValueError):
        UNet(n_classes=33)
    with pytest.raises(ValueError):
        UNetABN(n_classes=0)
    a, b = torch_train.get_model('unet'), torch_train.get_model('unet_abn')
    assert type(a) is UNet and type(b) is UNetABN and a.num_classes == 1 and b.num_classes == 1
    assert isinstance(b.inc.conv.conv[1], InPlaceABN) and b.inc.conv.conv[1].activation == 'leaky_relu'
    assert a.inc.conv.conv[0].weight.shape == (32, 3, 3, 3) and isinstance(a.finaldrop, torch.nn.Dropout2d) and a.finaldrop.p == 0.5
    ab = Afterburner()
    assert type(ab.unet) is UNet and ab.unet.inc.conv.conv[0].weight.shape == (32, 1, 3, 3) and ab.unet.outc.conv.weight.shape == (1, 32, 1, 1)
    assert all(k.startswith('unet.') for k in ab.state_dict()) and len(ab.state_dict()) == 18 * 7 + 2


def test_afterburner_equals_its_unet_on_the_fixture(emulated):
    """Afterburner(1) loaded from the g1_ case under the ``unet.`` prefix: the same network, the same result"""
    g = load_case('g1')
    mc.check_product_golden(make_afterburner(g), AfterburnerCase(g), 'cpu')


class AfterburnerCase(object):
    """a fixture case seen through Afterburner's ``unet.`` prefix (gradient and buffer names)"""

    def __init__(self, g):
        self.g = g
        self.files = [self._out(k) for k in g.files]

    @staticmethod
    def _out(k):
        for head in ('gidx/', 'gval/', 'buf/'):
            if k.startswith(head):
                return head + 'unet.' + k[len(head):]
        return k

    def __getitem__(self, k):
        for head in ('gidx/', 'gval/', 'buf/'):
            if k.startswith(head + 'unet.'):
                return self.g[head + k[len(head) + 5:]]
        v = self.g[k]
        return np.array(['unet.' + str(n) for n in v]) if k == 'grad_names' else v


def make_afterburner(g, n_filters=8):
    from lib.models.afterburner import Afterburner
    from lib.models.unet import UNet
    from oracle import fill
    ab = Afterburner(1)
    ab.unet = UNet(n_channels=1, n_classes=1, n_filters=n_filters)       # (the fixture's width; Afterburner's own is 32)
    ab.unet.finaldrop.p = 0.0
    sd = fill.seeded_state(ab.unet.state_dict(), int(g['seed']))
    assert ['unet.' + k for k in sd] == list(ab.state_dict())
    ab.load_state_dict({'unet.' + k: v for k, v in sd.items()})
    return ab


# ---- the operator alone ----------------------------------------------------------------------------------------------------
def make_probe_net(mode):
    """'chain': conv 1x1 (3 -> 12) = skip -> MaxPool2d(2) -> conv 1x1 (12 -> 12) -> upsample_nearest2x into the second slice
    of a [skip | up] concat buffer (padded slices 12 -> 16) -> conv 1x1 over the concat -> head.
    'frozen': the upsample reads the network input (needs_grad False: no backward launch); cat([conv 1x1 of it, it]) -> conv.
    'dangling': the chain's upsampled tensor is computed and nothing reads it (no gradient arrives); the last conv reads the skip.
    The views of the operator are kept in .probe."""
    from torch import nn
    from segnb.net import HipNet, concat, conv_unit, head_1x1, maxpool, upsample_nearest2x

    class ProbeNet(HipNet):
        def __init__(self):
            super(ProbeNet, self).__init__()
            self.c1 = nn.Conv2d(3, 12, 1)
            self.c2 = nn.Conv2d(12, 12, 1)
            self.c3 = nn.Conv2d({'chain': 24, 'frozen': 15, 'dangling': 12}[mode], 8, 1)
            self.head = nn.Conv2d(8, 1, 1)
            self.probe = {}
            self._init_engine(3)

        def _build(self, tape, x, dlogits):
            def conv(t, m, segs, tag, out=None):
                return conv_unit(tape, t, m.weight, m.bias, segs, stride=1, pad=0, act=nv.ACT_NONE, out=out, tag=tag)
            N, H, W = x.v.N, x.v.H, x.v.W
            if mode == 'frozen':
                cat = tape.view('cat', N, 2 * H, 2 * W, 16 + 8)
                u = upsample_nearest2x(tape, x, out=cat.slice(16, 8), tag='up')
                s = conv(u, self.c1, [(3, 8)], 'c1', out=cat.slice(0, 16))
                self.probe = dict(x=x.v, up=u.v)
                y = conv(concat(tape, [(s, 0), (u, 16)], cat), self.c3, [(12, 16), (3, 8)], 'c3')
                return head_1x1(tape, y, self.head.weight, self.head.bias, dlogits)
            cat = tape.view('cat', N, H, W, 32)
            s = conv(x, self.c1, [(3, 8)], 'c1', out=cat.slice(0, 16))
            z = conv(maxpool(tape, s, 2, 2, 0), self.c2, [(12, 16)], 'c2')
            if mode == 'dangling':
                d = upsample_nearest2x(tape, z, tag='dangling')
                self.probe = dict(z=z.v, up=d.v)
                y = conv(s, self.c3, [(12, 16)], 'c3')
                return head_1x1(tape, y, self.head.weight, self.head.bias, dlogits)
            u = upsample_nearest2x(tape, z, out=cat.slice(16, 16), tag='up')
            self.probe = dict(z=z.v, up=u.v, u=u, zact=z)
            y = conv(concat(tape, [(s, 0), (u, 16)], cat), self.c3, [(12, 16), (12, 16)], 'c3')
            return head_1x1(tape, y, self.head.weight, self.head.bias, dlogits)

    torch.manual_seed(11)
    return ProbeNet()


def probe_reference(m, mode, x, G):
    """float64 torch: -> (logits, {parameter name: gradient of (logits * G).sum()})"""
    import torch.nn.functional as F
    ps = {n: p.detach().cpu().double().requires_grad_(True) for n, p in m.named_parameters()}

    def conv(t, k):
        return F.conv2d(t, ps[k + '.weight'], ps[k + '.bias'])
    xd = x.double()
    if mode == 'frozen':
        u = F.interpolate(xd, scale_factor=2, mode='nearest')
        y = conv(torch.cat([conv(u, 'c1'), u], 1), 'c3')
    else:
        s = conv(xd, 'c1')
        z = conv(F.max_pool2d(s, 2), 'c2')
        y = conv(s if mode == 'dangling' else torch.cat([s, F.interpolate(z, scale_factor=2, mode='nearest')], 1), 'c3')
    lo = conv(y, 'head')
    (lo * G.double()).sum().backward()
    return lo.detach(), {n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in ps.items()}


def _count_calls(monkeypatch):
    calls, orig = [], nv.call

    def call(name, *a):
        calls.append(name)
        return orig(name, *a)
    monkeypatch.setattr(nv, 'call', call)
    return calls


def check_probe_net(mode, device, monkeypatch, dtype='f32', rtol=1e-4):
    """one step of the probe net against float64; -> (net, names of the ABI calls of the step).  rtol: of the logits' scale and
    of each gradient tensor's L2 norm."""
    m = make_probe_net(mode).set_compute_dtype(dtype).to(device).train()
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 3, 12, 20), generator=g)
    hw = (24, 40) if mode == 'frozen' else (12, 20)
    G = torch.randn((2, 1) + hw, generator=g)
    ref_lo, ref_g = probe_reference(m, mode, x, G)
    calls = _count_calls(monkeypatch)
    out = m(x.to(device))
    (out * G.to(device)).sum().backward()
    assert float((out.detach().cpu().double() - ref_lo).abs().max()) <= rtol * float(ref_lo.abs().max())
    for n, p in m.named_parameters():
        if float(ref_g[n].norm()) == 0.0:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            continue
        err = float((p.grad.detach().cpu().double() - ref_g[n]).norm() / ref_g[n].norm())
        assert err <= rtol, (mode, n, err)
    return m, calls


def test_operator_forward_copy_and_backward_scan_order_sum(monkeypatch, emulated):
    m, calls = check_probe_net('chain', 'cpu', monkeypatch)
    assert calls.count('segnb_upsample_nearest2x_fwd') == 1 and calls.count('segnb_upsample_nearest2x_bwd') == 1
    pv = m.probe
    z, up = pv['z'].dense(), pv['up'].dense()
    assert tuple(z.shape) == (2, 6, 10, 16) and tuple(up.shape) == (2, 12, 20, 16) and pv['up'].ld == 32
    assert torch.equal(up, R.nearest_fwd(z))
    # the backward read the concat gradient's second slice at the concat's stride and contributed the window sums
    gu, gz = pv['u'].g, pv['zact'].g
    assert gu.ld == 32 and torch.equal(gz.dense(), R.nearest_bwd(gu.dense()))


def test_operator_skips_its_backward_without_a_gradient_or_a_differentiable_input(monkeypatch, emulated):
    m, calls = check_probe_net('frozen', 'cpu', monkeypatch)
    assert calls.count('segnb_upsample_nearest2x_fwd') == 1 and calls.count('segnb_upsample_nearest2x_bwd') == 0
    assert torch.equal(m.probe['up'].dense(), R.nearest_fwd(m.probe['x'].dense()))
    monkeypatch.undo()
    m, calls = check_probe_net('dangling', 'cpu', monkeypatch)
    assert calls.count('segnb_upsample_nearest2x_fwd') == 1 and calls.count('segnb_upsample_nearest2x_bwd') == 0
    assert torch.equal(m.probe['up'].dense(), R.nearest_fwd(m.probe['z'].dense()))


def test_operator_refuses_an_output_view_of_another_size(emulated):
    from segnb.net import Act, Tape, upsample_nearest2x
    m = make_probe_net('chain')
    tape = Tape(m, torch.device('cpu'), 'f32')
    tape.begin(False, False)
    x = Act(tape.view('x', 1, 4, 4, 8), needs_grad=False)
    with pytest.raises(ValueError):
        upsample_nearest2x(tape, x, out=tape.view('o', 1, 8, 6, 8))


def test_emulator_launches_and_refusals():
    emu = R.UpsampleAbiEmulator()
    g = torch.Generator().manual_seed(2)
    for tdt, code in ((torch.float32, nv.F32), (torch.bfloat16, nv.BF16)):
        x = torch.randn((2, 3, 5, 24), generator=g).to(tdt)
        out = torch.full((2, 6, 10, 40), 7.0, dtype=tdt)
        assert emu.segnb_upsample_nearest2x_fwd(code, x.data_ptr(), 24, 2, 3, 5, 16, out.data_ptr(), 40, None) == 0
        assert torch.equal(out[..., :16], R.nearest_fwd(x[..., :16])) and bool((out[..., 16:] == 7.0).all())
        go = torch.randn((2, 6, 10, 40), generator=g).to(tdt)
        dx = torch.full((2, 3, 5, 24), 7.0, dtype=tdt)
        assert emu.segnb_upsample_nearest2x_bwd(code, go.data_ptr(), 40, 2, 3, 5, 16, dx.data_ptr(), 24, None) == 0
        u = go[..., :16].float()
        want = (((u[:, 0::2, 0::2] + u[:, 0::2, 1::2]) + u[:, 1::2, 0::2]) + u[:, 1::2, 1::2]).to(tdt)
        assert torch.equal(dx[..., :16], want) and bool((dx[..., 16:] == 7.0).all())
        assert emu.segnb_upsample_nearest2x_fwd(code, x.data_ptr(), 24, 2, 3, 5, 12, out.data_ptr(), 40, None) == -1
        assert emu.segnb_upsample_nearest2x_fwd(code, x.data_ptr(), 8, 2, 3, 5, 16, out.data_ptr(), 40, None) == -1
        assert emu.segnb_upsample_nearest2x_bwd(code, None, 40, 2, 3, 5, 16, dx.data_ptr(), 24, None) == -1


# ---- the ABI triple ----------------------------------------------------------------------------------------------------------
def test_upsample_abi_triple():
    hdr = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    names = set(re.findall(r'\b(segnb_\w+)\s*\(', hdr))
    assert names == UP_NAMES and set(nv.UP_SIGNATURES) == names
    others = (set(nv.SIGNATURES) | set(nv.PLAIN) | set(nv.MC_SIGNATURES) | set(nv.MC_PLAIN) | set(nv.GCN_SIGNATURES)
              | set(nv.GCN_PLAIN) | set(nv.ELU_SIGNATURES) | set(nv.ELU_PLAIN))
    assert not (names & others)
    emu = R.UpsampleAbiEmulator()
    assert {m for m in dir(emu) if m.startswith('segnb_upsample_nearest')} == names
    for name, args in re.findall(r'\bint\s+(segnb_\w+)\s*\(([^)]*)\)', hdr):
        n = len([a for a in args.split(',') if a.strip()])
        assert len(nv.UP_SIGNATURES[name]) == n, (name, n)
        # the argument order of the bilinear pair
        assert nv.UP_SIGNATURES[name] == nv.SIGNATURES[name.replace('nearest', 'bilinear')]


def test_library_exports_the_upsample_entry_points_and_refuses_on_the_host():
    assert os.path.exists(nv.LIB_PATH), 'libsegnb_hip.so not built (run __graft_entry__.build())'
    lib = ctypes.CDLL(nv.LIB_PATH)
    assert not [n for n in sorted(UP_NAMES) if not hasattr(lib, n)]
    # the refusals are host code: they answer before anything is launched
    lib.segnb_last_error.restype = ctypes.c_char_p
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    p += (-p) % 16
    P = ctypes.c_void_p
    for name in sorted(UP_NAMES):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ctypes.c_int, nv.UP_SIGNATURES[name]
        for args, word in (((nv.BF16, P(p), 16, 1, 2, 2, 12, P(p + 2048), 16, None), 'Cp % 8'),
                           ((nv.BF16, P(p), 8, 1, 2, 2, 16, P(p + 2048), 16, None), 'stride'),
                           ((nv.BF16, P(p), 16, 1, 2, 2, 16, P(p + 2048), 8, None), 'stride'),
                           ((nv.BF16, P(p), 20, 1, 2, 2, 16, P(p + 2048), 16, None), 'stride'),
                           ((nv.BF16, None, 16, 1, 2, 2, 16, P(p + 2048), 16, None), 'NULL'),
                           ((nv.BF16, P(p), 16, 1, 2, 2, 16, None, 16, None), 'NULL'),
                           ((nv.BF16, P(p), 16, 1, 2, 2, 16, P(p), 16, None), 'alias'),
                           ((nv.BF16, P(p + 2), 16, 1, 2, 2, 16, P(p + 2048), 16, None), 'aligned'),
                           ((nv.F32, P(p), 8, 1 << 9, 1 << 9, 1 << 9, 8, P(p + 2048), 8, None), 'int32'),
                           ((7, P(p), 16, 1, 2, 2, 16, P(p + 2048), 16, None), 'dtype')):
            assert fn(*args) == -1, (name, args)
            msg = lib.segnb_last_error().decode()
            assert name in msg and word in msg, (name, word, msg)
