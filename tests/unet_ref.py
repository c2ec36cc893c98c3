"""Float64-capable CPU restatement of UNet / UNetABN and of the nearest-upsample ABI (include/segnb_upsample.h) -- TEST
INFRASTRUCTURE ONLY.

``forward(sd, x, ...)`` restates the reference's UNet.forward (lib/models/unet.py:95-107; unet_abn.py has the same graph with
InPlaceABN = BatchNorm + LeakyReLU(0.01) in double_conv) with torch functional ops on the model's state_dict keys, in the dtype
of its arguments.  ``nearest_fwd`` / ``nearest_bwd`` restate the two launches on torch tensors (the formulas of the header,
rounding included); ``UpsampleAbiEmulator`` exposes them on raw host memory the way oracle.abi_emulator.AbiEmulator does for
segnb_hip.h, so the product's host code (segnb.net.upsample_nearest2x, lib.models.unet) runs on the CPU against the fixture.
"""
import torch
import torch.nn.functional as F

from oracle.abi_emulator import AbiEmulator, _nhwc, _tdt
from squeezenet_ref import gather_up

F64 = torch.float64
ABN_SLOPE = 0.01
CASES = {                      # prefix -> (model, constructor arguments): tests/golden/make_golden_unet.py
    'sq': ('UNet', {}),
    'ns': ('UNet', {}),
    'dc': ('UNet', {'upsample': False}),
    'g1': ('UNet', {'n_channels': 1}),
    'abn': ('UNetABN', {}),
}


def _double(sd, p, x, train, abn):
    """double_conv under the key prefix p (its nn.Sequential): UNet conv.0 / .1 (BatchNorm) / .3 / .4, UNetABN conv.0 .. conv.3"""
    for ci, ni in ((0, 1), (2, 3)) if abn else ((0, 1), (3, 4)):
        c, n = '%s.%d' % (p, ci), '%s.%d' % (p, ni)
        x = F.conv2d(x, sd[c + '.weight'], sd[c + '.bias'], padding=1)
        # (training mode updates the running statistics in sd, as the module does)
        x = F.batch_norm(x, sd[n + '.running_mean'], sd[n + '.running_var'], sd[n + '.weight'], sd[n + '.bias'], train, 0.1, 1e-5)
        x = F.leaky_relu(x, ABN_SLOPE) if abn else F.relu(x)
    return x


def forward(sd, x, train=True, upsample=True, abn=False, drop=None):
    """UNet.forward / UNetABN.forward on a state_dict.  drop: optional [N, C] multiplier table for finaldrop (0 or 1 / (1 - p)
    per image and channel, what Dropout2d draws); None: no dropout."""
    x1 = _double(sd, 'inc.conv.conv', x, train, abn)
    x2 = _double(sd, 'down1.mpconv.1.conv', F.max_pool2d(x1, 2), train, abn)
    x3 = _double(sd, 'down2.mpconv.1.conv', F.max_pool2d(x2, 2), train, abn)
    x4 = _double(sd, 'down3.mpconv.1.conv', F.max_pool2d(x3, 2), train, abn)
    h = _double(sd, 'down4.mpconv.1.conv', F.max_pool2d(x4, 2), train, abn)
    for k, skip in zip((1, 2, 3, 4), (x4, x3, x2, x1)):
        p = 'up%d' % k
        if upsample:
            h = F.interpolate(h, scale_factor=2, mode='nearest')
        else:
            h = F.conv_transpose2d(h, sd[p + '.up.weight'], sd[p + '.up.bias'], stride=2)
        h = _double(sd, p + '.conv.conv', torch.cat([skip, h], 1), train, abn)
    if drop is not None:
        h = h * drop.to(h.dtype)[:, :h.shape[1], None, None]
    return F.conv2d(h, sd['outc.conv.weight'], sd['outc.conv.bias'])


def forward_for(prefix):
    """-> f(sd, x, train=True, drop=None) for a fixture case"""
    name, kw = CASES[prefix]
    return lambda sd, x, train=True, drop=None: forward(sd, x, train, kw.get('upsample', True), name == 'UNetABN', drop)


# ---- the two launches of include/segnb_upsample.h on [N, H, W, C] tensors of the storage dtype ---------------------------------
def nearest_fwd(x):
    """[N, H, W, C] -> [N, 2H, 2W, C]: a copy"""
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)


def nearest_bwd(g):
    """[N, 2H, 2W, C] -> [N, H, W, C]: the window's four gradients in scan order in fp32, rounded once"""
    return gather_up(g).to(g.dtype)


class UpsampleAbiEmulator(AbiEmulator):
    """AbiEmulator + the entry points of include/segnb_upsample.h, on raw host memory (CPU tensors)."""

    @staticmethod
    def _refused(dtype, lo, ld_lo, hi, ld_hi, N, H, W, Cp):
        return (dtype not in (0, 1) or N < 1 or H < 1 or W < 1 or Cp < 8 or Cp % 8 or 16 * N * H * W >= 2 ** 31 or not lo or not hi
                or ld_lo < Cp or ld_hi < Cp or ld_lo % 8 or ld_hi % 8 or lo == hi)

    def segnb_upsample_nearest2x_fwd(self, dtype, x, ld_x, N, H, W, Cp, out, ld_out, stream):
        if self._refused(dtype, x, ld_x, out, ld_out, N, H, W, Cp):
            return -1
        dt = _tdt(dtype)
        _nhwc(out, N, 2 * H, 2 * W, Cp, ld_out, dt).copy_(nearest_fwd(_nhwc(x, N, H, W, Cp, ld_x, dt)))
        return 0

    def segnb_upsample_nearest2x_bwd(self, dtype, g_out, ld_go, N, H, W, Cp, dx, ld_dx, stream):
        if self._refused(dtype, dx, ld_dx, g_out, ld_go, N, H, W, Cp):
            return -1
        dt = _tdt(dtype)
        _nhwc(dx, N, H, W, Cp, ld_dx, dt).copy_(nearest_bwd(_nhwc(g_out, N, 2 * H, 2 * W, Cp, ld_go, dt)))
        return 0
