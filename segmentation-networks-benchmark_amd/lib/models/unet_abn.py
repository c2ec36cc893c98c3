"""UNetABN on the MI355X engine -- drop-in for the reference's ``lib.models.unet_abn.UNetABN`` (lib/models/unet_abn.py:6-107):
the graph of ``lib.models.unet.UNet`` with ``lib.modules.abn.InPlaceABN`` in ``double_conv`` (state_dict keys ``conv.0`` ..
``conv.3``).  The activation and its slope come from the module, as in LinkNet34's decoder; both affine forms of InPlaceABN run
through conv_unit's ``abs_form`` handling.
"""
from torch import nn

from lib.models import unet as _unet
from lib.modules.abn import ACT_LEAKY_RELU, ACT_NONE, InPlaceABN
from segnb import _native as nv


def _abn_act(abn):
    if abn.activation == ACT_LEAKY_RELU:
        return nv.ACT_LEAKY, abn.slope
    if abn.activation == ACT_NONE:
        return nv.ACT_NONE, 0.0
    raise ValueError('UNetABN: InPlaceABN activation %r is not served by the fused convolution units' % (abn.activation,))


class double_conv(nn.Module):
    '''(conv => InPlaceABN) * 2'''

    def __init__(self, in_ch, out_ch):
        super(double_conv, self).__init__()
        self.conv = nn.Sequential(
            nn.Conv2d(in_ch, out_ch, 3, padding=1),
            InPlaceABN(out_ch),
            nn.Conv2d(out_ch, out_ch, 3, padding=1),
            InPlaceABN(out_ch),
        )
    forward = _unet._holder_forward

    def units(self):
        c = self.conv
        return [(c[0], c[1]) + _abn_act(c[1]), (c[2], c[3]) + _abn_act(c[3])]


class inconv(_unet.inconv):
    _block = double_conv


class down(_unet.down):
    _block = double_conv


class up(_unet.up):
    _block = double_conv


outconv = _unet.outconv


class UNetABN(_unet.UNet):
    _parts = (inconv, down, up, outconv)
