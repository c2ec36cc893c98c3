"""SqueezeNet on the MI355X engine -- drop-in for the reference's ``lib.models.squeezenet.SqueezeNet``
(lib/models/squeezenet.py:68-151): ``SqueezeNet(in_channels=3, num_classes=1)``, same attribute tree / state_dict keys
(``conv1.weight``, ``fire2.squeeze.weight``, ``conv10.0.weight``, ``dfire2.squeeze.bias``, ``dconv1.bias``: 104 tensors), torch's
default Conv2d initialisation (the reference sets none), fp32 NCHW logits at the input size.

Plan (segnb.net): every convolution is a conv_unit with bias and NO activation; nn.ELU is the executor's ``elu`` pass
(csrc/elu.hip behind include/segnb_elu.h), in place on the convolution's output.  A Fire block's two expand convolutions write
the two channel slices of one buffer (zero-copy torch.cat) and ONE ELU pass runs over the whole buffer; in the backward that
pass writes both convolutions' gradients and bias-gradient sums.  The three ``F.upsample(d, 2, 'nearest') + skip`` sites
(squeezenet.py:137-149) ride on the ELU pass of the DFire block in front of them (``elu(up_skip=...)``).  MaxPool2d(2) is the
executor's maxpool; the 1 x 1 classifier runs on the head kernels.
"""
from torch import nn

from segnb import _native as nv
from segnb import convplan as cp
from segnb.net import HipNet, concat, conv_unit, elu, head_1x1, maxpool


def _holder_forward(self, *a, **k):
    raise RuntimeError('parameter holder; run the whole SqueezeNet (HIP executor)')


class Fire(nn.Module):
    """squeeze 1x1 -> ELU -> cat(expand1x1, expand3x3) -> ELU (squeezenet.py:7-27)"""

    def __init__(self, inplanes, squeeze_planes, expand1x1_planes, expand3x3_planes):
        super(Fire, self).__init__()
        self.inplanes = inplanes
        self.squeeze = nn.Conv2d(inplanes, squeeze_planes, kernel_size=1)
        self.squeeze_activation = nn.ELU(inplace=True)
        self.expand1x1 = nn.Conv2d(squeeze_planes, expand1x1_planes, kernel_size=1)
        self.expand1x1_activation = nn.ELU(inplace=True)
        self.expand3x3 = nn.Conv2d(squeeze_planes, expand3x3_planes, kernel_size=3, padding=1)
        self.expand3x3_activation = nn.ELU(inplace=True)
    forward = _holder_forward


class DFire(nn.Module):
    """cat(expand1x1, expand3x3) -> ELU -> squeeze 1x1 -> ELU (squeezenet.py:29-52)"""

    def __init__(self, inplanes, squeeze_planes, expand1x1_planes, expand3x3_planes):
        super(DFire, self).__init__()
        self.inplanes = inplanes
        self.expand1x1 = nn.Conv2d(inplanes, expand1x1_planes, kernel_size=1)
        self.expand1x1_activation = nn.ELU(inplace=True)
        self.expand3x3 = nn.Conv2d(inplanes, expand3x3_planes, kernel_size=3, padding=1)
        self.expand3x3_activation = nn.ELU(inplace=True)
        self.squeeze = nn.Conv2d(expand3x3_planes + expand1x1_planes, squeeze_planes, kernel_size=1)
        self.squeeze_activation = nn.ELU(inplace=True)
    forward = _holder_forward


class SharpMaskBypass(nn.Module):
    """Defined by the reference (squeezenet.py:54-65) and used by nothing in it; kept for the surface."""

    def __init__(self, enc_features, dec_features, num_classes):
        super(SharpMaskBypass, self).__init__()
        self.conv1 = nn.Sequential(nn.Conv2d(enc_features, 32, kernel_size=3, padding=1), nn.ELU(inplace=True))
        self.conv2 = nn.Sequential(nn.Conv2d(32 + dec_features, num_classes, kernel_size=3, padding=1), nn.ELU(inplace=True))
    forward = _holder_forward


def _seg(c):
    return [(c, cp.pad8(c))]


def _conv(tape, x, m, tag, out=None):
    return conv_unit(tape, x, m.weight, m.bias, _seg(m.in_channels), stride=1, pad=m.padding[0], act=nv.ACT_NONE, out=out, tag=tag)


def _expand(tape, blk, x, tag):
    """ELU(cat(expand1x1(x), expand3x3(x))): the two convolutions write the slices of one view, one ELU pass over it"""
    xv = x.v
    c1, c3 = blk.expand1x1.out_channels, blk.expand3x3.out_channels
    cat = tape.view(tape.site(tag + '.cat'), xv.N, xv.H, xv.W, c1 + c3)
    e1 = _conv(tape, x, blk.expand1x1, tag + '.e1', out=cat.slice(0, c1))
    e3 = _conv(tape, x, blk.expand3x3, tag + '.e3', out=cat.slice(c1, c3))
    return elu(tape, concat(tape, [(e1, 0), (e3, c1)], cat), tag=tag + '.elu')


def fire(tape, blk, x, tag):
    s = elu(tape, _conv(tape, x, blk.squeeze, tag + '.sq'), tag=tag + '.sq.elu')
    return _expand(tape, blk, s, tag)


def dfire(tape, blk, x, tag, up_skip=None):
    """-> the block's output, or with up_skip: F.upsample(output, 2, 'nearest') + up_skip"""
    e = _expand(tape, blk, x, tag)
    s = elu(tape, _conv(tape, e, blk.squeeze, tag + '.sq'), up_skip=up_skip, tag=tag + '.sq.elu')
    return s[1] if up_skip is not None else s


class SqueezeNet(HipNet):
    # conv1 and the outputs of fire4 / fire8 feed a pooling and a skip add: their two gradients go to the producing pass as two
    # sources (segnb.net.Tape.lazy_add); no gradient view of this model is a slice another tensor accumulates into
    lazy_add = True

    def __init__(self, in_channels=3, num_classes=1):
        super(SqueezeNet, self).__init__()
        if in_channels != 3:
            raise ValueError('SqueezeNet supports 3 input channels, got %d' % in_channels)
        if not 1 <= num_classes <= 32:
            raise ValueError('SqueezeNet supports 1..32 classes (the head kernels, segnb_head_fwd), got %d' % num_classes)
        self.num_classes = num_classes
        self.conv1 = nn.Conv2d(in_channels, 96, kernel_size=3, padding=1)
        self.pool1 = nn.MaxPool2d(2, 2)
        self.fire2 = Fire(96, 16, 64, 64)
        self.fire3 = Fire(128, 16, 64, 64)
        self.pool3 = nn.MaxPool2d(2, 2)
        self.fire4 = Fire(128, 48, 128, 128)
        self.fire5 = Fire(256, 48, 128, 128)
        self.pool5 = nn.MaxPool2d(2, 2)
        self.fire6 = Fire(256, 48, 192, 192)
        self.fire7 = Fire(384, 48, 192, 192)
        self.fire8 = Fire(384, 64, 256, 256)
        self.fire9 = Fire(512, 64, 256, 256)
        self.conv10 = nn.Sequential(nn.Conv2d(512, 1024, kernel_size=1), nn.ELU(inplace=True))
        self.dconv10 = nn.Sequential(nn.Conv2d(1024, 512, kernel_size=1), nn.ELU(inplace=True))
        self.dfire9 = DFire(512, 512, 256, 256)
        self.dfire8 = DFire(512, 384, 256, 256)
        self.dfire7 = DFire(384, 384, 192, 192)
        self.dfire6 = DFire(384, 256, 192, 192)
        self.dfire5 = DFire(256, 256, 128, 128)
        self.dfire4 = DFire(256, 128, 128, 128)
        self.dfire3 = DFire(128, 128, 64, 64)
        self.dfire2 = DFire(128, 96, 48, 48)
        self.dconv1 = nn.Conv2d(96, num_classes, kernel_size=1)
        self._init_engine(in_channels)

    def _check_input(self, x):
        super(SqueezeNet, self)._check_input(x)
        if x.shape[2] % 8 or x.shape[3] % 8:
            raise ValueError('SqueezeNet needs H and W divisible by 8 (three 2x2 poolings, three x2 upsamples added to '
                             'their skips), got %dx%d' % (x.shape[2], x.shape[3]))

    def _build(self, tape, x, dlogits):
        conv1 = _conv(tape, x, self.conv1, 'conv1')                       # (no activation: squeezenet.py:118)
        h = maxpool(tape, conv1, 2, 2, 0, tag='pool1')
        h = fire(tape, self.fire2, h, 'fire2')
        h = fire(tape, self.fire3, h, 'fire3')
        fire4 = fire(tape, self.fire4, h, 'fire4')
        h = maxpool(tape, fire4, 2, 2, 0, tag='pool3')
        for name in ('fire5', 'fire6', 'fire7'):
            h = fire(tape, getattr(self, name), h, name)
        fire8 = fire(tape, self.fire8, h, 'fire8')
        h = maxpool(tape, fire8, 2, 2, 0, tag='pool5')
        h = fire(tape, self.fire9, h, 'fire9')
        h = elu(tape, _conv(tape, h, self.conv10[0], 'conv10'), tag='conv10.elu')
        h = elu(tape, _conv(tape, h, self.dconv10[0], 'dconv10'), tag='dconv10.elu')
        h = dfire(tape, self.dfire9, h, 'dfire9', up_skip=fire8)
        for name in ('dfire8', 'dfire7', 'dfire6'):
            h = dfire(tape, getattr(self, name), h, name)
        h = dfire(tape, self.dfire5, h, 'dfire5', up_skip=fire4)
        h = dfire(tape, self.dfire4, h, 'dfire4')
        h = dfire(tape, self.dfire3, h, 'dfire3')
        h = dfire(tape, self.dfire2, h, 'dfire2', up_skip=conv1)
        # dconv1 (squeezenet.py:102, 149): a 1 x 1 classifier over 96 channels, 1..32 classes: the head kernels serve it
        return head_1x1(tape, h, self.dconv1.weight, self.dconv1.bias, dlogits, tag='dconv1')
