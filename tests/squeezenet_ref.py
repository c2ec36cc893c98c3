"""Float64 CPU restatement of SqueezeNet and of the ELU ABI (include/segnb_elu.h) -- TEST INFRASTRUCTURE ONLY.

``forward(sd, x)`` restates the reference's SqueezeNet.forward (lib/models/squeezenet.py:117-151) with torch functional ops on
the model's state_dict keys, in the dtype of its arguments.  ``elu_fwd`` / ``elu_bwd`` restate the two launches on torch
tensors (the formulas of the header, rounding included); ``EluAbiEmulator`` exposes them on raw host memory the way
oracle.abi_emulator.AbiEmulator does for segnb_hip.h, so the product's host code (segnb.net.elu, lib.models.squeezenet) runs on
CPU against the fixture.
"""
import torch
import torch.nn.functional as F

from oracle.abi_emulator import REPL, AbiEmulator, _mem, _nhwc, _tdt

F64 = torch.float64
FIRES = ['fire%d' % i for i in range(2, 10)]
DFIRES = ['dfire%d' % i for i in range(9, 1, -1)]


def _conv(sd, p, x, pad=0):
    return F.conv2d(x, sd[p + '.weight'], sd[p + '.bias'], padding=pad)


def _expand(sd, p, x):
    return torch.cat([F.elu(_conv(sd, p + '.expand1x1', x)), F.elu(_conv(sd, p + '.expand3x3', x, 1))], 1)


def fire(sd, p, x):
    return _expand(sd, p, F.elu(_conv(sd, p + '.squeeze', x)))


def dfire(sd, p, x):
    return F.elu(_conv(sd, p + '.squeeze', _expand(sd, p, x)))


def up2(x):
    return F.interpolate(x, scale_factor=2, mode='nearest')


def forward(sd, x):
    """SqueezeNet.forward (squeezenet.py:117-151) on its state_dict"""
    conv1 = _conv(sd, 'conv1', x, 1)
    h = F.max_pool2d(conv1, 2, 2)
    h = fire(sd, 'fire2', h)
    h = fire(sd, 'fire3', h)
    fire4 = fire(sd, 'fire4', h)
    h = F.max_pool2d(fire4, 2, 2)
    for p in ('fire5', 'fire6', 'fire7'):
        h = fire(sd, p, h)
    fire8 = fire(sd, 'fire8', h)
    h = F.max_pool2d(fire8, 2, 2)
    h = fire(sd, 'fire9', h)
    h = F.elu(_conv(sd, 'dconv10.0', F.elu(_conv(sd, 'conv10.0', h))))
    h = up2(dfire(sd, 'dfire9', h)) + fire8
    for p in ('dfire8', 'dfire7', 'dfire6', 'dfire5'):
        h = dfire(sd, p, h)
    h = up2(h) + fire4
    for p in ('dfire4', 'dfire3', 'dfire2'):
        h = dfire(sd, p, h)
    return _conv(sd, 'dconv1', up2(h) + conv1)


# ---- the two launches of include/segnb_elu.h on [N, H, W, C] tensors of the storage dtype ---------------------------------
def elu_fwd(z, up_skip=None):
    """-> (a, up or None): a = rnd(elu(z)) with fp32 arithmetic; up = rnd(float(a) + float(up_skip)) on the nearest x2 grid"""
    zf = z.float()
    a = torch.where(zf > 0, zf, torch.expm1(zf)).to(z.dtype)
    if up_skip is None:
        return a, None
    rep = a.float().repeat_interleave(2, 1).repeat_interleave(2, 2)
    return a, (rep + up_skip.float()).to(z.dtype)


def gather_up(g_up):
    """the four gradients of a 2x2 window, summed in scan order in fp32: [N, 2H, 2W, C] -> [N, H, W, C]"""
    u = g_up.float()
    return ((u[:, 0::2, 0::2] + u[:, 0::2, 1::2]) + u[:, 1::2, 0::2]) + u[:, 1::2, 1::2]


def elu_bwd(a, g_direct=None, g_add=None, g_up=None):
    """-> dz = rnd(g * (a > 0 ? 1 : a + 1)), g = g_direct + g_add + window sum of g_up in fp32, in that order"""
    g = None
    for t in (g_direct, g_add):
        if t is not None:
            g = t.float() if g is None else g + t.float()
    if g_up is not None:
        w4 = gather_up(g_up)
        g = w4 if g is None else g + w4
    af = a.float()
    return (g * torch.where(af > 0, torch.ones_like(af), af + 1.0)).to(a.dtype)


class EluAbiEmulator(AbiEmulator):
    """AbiEmulator + the entry points of include/segnb_elu.h, on raw host memory (CPU tensors)."""

    def segnb_elu_ok(self, dtype, N, H, W, Cp):
        if dtype not in (0, 1) or N < 1 or H < 1 or W < 1:
            return 0
        if Cp < 8 or Cp > 1024 or Cp % 8:
            return 0
        return 1 if 16 * N * H * W < 2 ** 31 else 0

    def segnb_elu_fwd(self, dtype, z, ld_z, N, H, W, Cp, a, ld_a, up_skip, ld_skip, up_out, ld_up, stream):
        if not self.segnb_elu_ok(dtype, N, H, W, Cp) or not z or not a or bool(up_skip) != bool(up_out):
            return -1
        dt = _tdt(dtype)
        S = _nhwc(up_skip, N, 2 * H, 2 * W, Cp, ld_skip, dt).clone() if up_skip else None
        av, up = elu_fwd(_nhwc(z, N, H, W, Cp, ld_z, dt).clone(), S)
        _nhwc(a, N, H, W, Cp, ld_a, dt).copy_(av)
        if up is not None:
            _nhwc(up_out, N, 2 * H, 2 * W, Cp, ld_up, dt).copy_(up)
        return 0

    def segnb_elu_bwd(self, dtype, a, ld_a, N, H, W, Cp, g_direct, ld_gd, g_add, ld_ga, g_up, ld_gu, dz, ld_dz, sums0, C0p,
                      sums1, stream):
        if not self.segnb_elu_ok(dtype, N, H, W, Cp) or not a or not dz or not (g_direct or g_add or g_up):
            return -1
        if sums0 and not (8 <= C0p <= Cp and C0p % 8 == 0 and bool(sums1) == (C0p < Cp)):
            return -1
        if sums1 and not sums0:
            return -1
        dt = _tdt(dtype)
        gd = _nhwc(g_direct, N, H, W, Cp, ld_gd, dt).clone() if g_direct else None
        ga = _nhwc(g_add, N, H, W, Cp, ld_ga, dt) if g_add else None
        gu = _nhwc(g_up, N, 2 * H, 2 * W, Cp, ld_gu, dt) if g_up else None
        d = elu_bwd(_nhwc(a, N, H, W, Cp, ld_a, dt), gd, ga, gu)
        _nhwc(dz, N, H, W, Cp, ld_dz, dt).copy_(d)
        if sums0:
            tot = d.double().reshape(-1, Cp).sum(0)
            _mem(sums0, REPL * 2 * C0p, F64).view(REPL, 2, C0p)[0, 0] += tot[:C0p]
            if sums1:
                C1 = Cp - C0p
                _mem(sums1, REPL * 2 * C1, F64).view(REPL, 2, C1)[0, 0] += tot[C0p:]
        return 0
