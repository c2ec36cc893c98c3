"""UNet on the MI355X engine -- drop-in for the reference's ``lib.models.unet.UNet`` (lib/models/unet.py:6-107):
``UNet(n_channels=3, n_classes=1, n_filters=32, upsample=True)``, the reference's classes ``double_conv``, ``inconv``, ``down``,
``up``, ``outconv`` as parameter holders, same attribute tree / state_dict keys (``inc.conv.conv.0.weight``,
``down1.mpconv.1.conv.4.running_var``, ``up1.conv.conv.1.num_batches_tracked``, ``outc.conv.bias``; ``up1.up.weight`` with
``upsample=False``), torch's default initialisation (the reference sets none), fp32 NCHW logits at the input size.

Plan (segnb.net): every ``double_conv`` is two conv_units (3x3, pad 1, bias, BatchNorm, activation).  The second unit of
``inc`` and ``down1..down3`` pools in the same pass (MaxPool2d(2) of the next ``down``) and writes its full-resolution output
straight into the skip slice of that level's concat buffer; ``up`` fills the other slice -- ``upsample_nearest2x``
(csrc/elementwise.hip behind include/segnb_upsample.h), or the ConvTranspose2d(C, C, 2, stride=2) as a conv_unit -- and
``torch.cat([skip, up])`` (unet.py:65) is zero-copy.  ``finaldrop`` is the Dropout2d multiplier table of the last unit; ``outc``
runs on the head kernels.

H and W must be multiples of 16: for other sizes the reference's ``F.pad`` with negative amounts (unet.py:61-64) crops the skip
tensors and returns logits smaller than the input (24x40 in, 16x32 out), which no loss accepts.
"""
from torch import nn

from segnb import _native as nv
from segnb import convplan as cp
from segnb.net import HipNet, concat, conv_unit, head_1x1, upsample_nearest2x


def _holder_forward(self, *a, **k):
    raise RuntimeError('parameter holder; run the whole UNet (HIP executor)')


class double_conv(nn.Module):
    '''(conv => BN => ReLU) * 2'''

    def __init__(self, in_ch, out_ch):
        super(double_conv, self).__init__()
        self.conv = nn.Sequential(
            nn.Conv2d(in_ch, out_ch, 3, padding=1),
            nn.BatchNorm2d(out_ch),
            nn.ReLU(inplace=True),
            nn.Conv2d(out_ch, out_ch, 3, padding=1),
            nn.BatchNorm2d(out_ch),
            nn.ReLU(inplace=True)
        )
    forward = _holder_forward

    def units(self):
        """[(convolution, normalisation, activation code, slope)] of the two units"""
        c = self.conv
        return [(c[0], c[1], nv.ACT_RELU, 0.0), (c[3], c[4], nv.ACT_RELU, 0.0)]


class inconv(nn.Module):
    _block = double_conv

    def __init__(self, in_ch, out_ch):
        super(inconv, self).__init__()
        self.conv = self._block(in_ch, out_ch)
    forward = _holder_forward


class down(nn.Module):
    _block = double_conv

    def __init__(self, in_ch, out_ch):
        super(down, self).__init__()
        self.mpconv = nn.Sequential(
            nn.MaxPool2d(2),
            self._block(in_ch, out_ch)
        )
    forward = _holder_forward


class up(nn.Module):
    _block = double_conv

    def __init__(self, in_ch, out_ch, upsample=True):
        super(up, self).__init__()
        if upsample:
            self.up = nn.Upsample(scale_factor=2, mode='nearest')
        else:
            self.up = nn.ConvTranspose2d(in_ch // 2, in_ch // 2, 2, stride=2)
        self.conv = self._block(in_ch, out_ch)
    forward = _holder_forward


class outconv(nn.Module):
    def __init__(self, in_ch, out_ch):
        super(outconv, self).__init__()
        self.conv = nn.Conv2d(in_ch, out_ch, 1)
    forward = _holder_forward


def _seg(c):
    return (c, cp.pad8(c))


def _double(tape, x, block, segs, tag, out=None, pool=False, dropmul=None):
    """the two units of a double_conv; out / pool / dropmul belong to the second one.  -> Act, or (Act, pooled Act)"""
    (c1, n1, a1, s1), (c2, n2, a2, s2) = block.units()
    mid = conv_unit(tape, x, c1.weight, c1.bias, segs, bn=n1, act=a1, slope=s1, tag=tag + '.c1')
    return conv_unit(tape, mid, c2.weight, c2.bias, [_seg(c1.out_channels)], bn=n2, act=a2, slope=s2, dropmul=dropmul, out=out,
                     pool=pool, tag=tag + '.c2')


class UNet(HipNet):
    _parts = (inconv, down, up, outconv)

    def __init__(self, n_channels=3, n_classes=1, n_filters=32, upsample=True):
        super(UNet, self).__init__()
        if not 1 <= n_classes <= 32:
            raise ValueError('%s supports 1..32 classes (the head kernels, segnb_head_fwd), got %d' % (type(self).__name__, n_classes))
        inconv_, down_, up_, outconv_ = self._parts
        self.num_classes = n_classes
        self.inc = inconv_(n_channels, n_filters)
        self.down1 = down_(n_filters, n_filters * 2)
        self.down2 = down_(n_filters * 2, n_filters * 4)
        self.down3 = down_(n_filters * 4, n_filters * 8)
        self.down4 = down_(n_filters * 8, n_filters * 8)
        self.up1 = up_(n_filters * 16, n_filters * 4, upsample=upsample)
        self.up2 = up_(n_filters * 8, n_filters * 2, upsample=upsample)
        self.up3 = up_(n_filters * 4, n_filters, upsample=upsample)
        self.up4 = up_(n_filters * 2, n_filters, upsample=upsample)
        self.finaldrop = nn.Dropout2d(p=0.5)
        self.outc = outconv_(n_filters, n_classes)
        self._nf, self._nch = n_filters, n_channels
        self._init_engine(n_channels)

    def _check_input(self, x):
        super(UNet, self)._check_input(x)
        if x.shape[2] % 16 or x.shape[3] % 16:
            raise ValueError('%s needs H and W divisible by 16 (four 2x2 poolings, four x2 upsamples concatenated with their '
                             'skips), got %dx%d' % (type(self).__name__, x.shape[2], x.shape[3]))

    def _build(self, tape, x, dlogits):
        nf, N, H, W = self._nf, x.v.N, x.v.H, x.v.W
        skip_c = [nf, nf * 2, nf * 4, nf * 8]             # x1 .. x4; the upsampled tensor beside x_k has as many channels
        # concat buffers [skip | up] at levels 0..3 (unet.py:65)
        cats = [tape.view('cat%d' % k, N, H >> k, W >> k, 2 * cp.pad8(c)) for k, c in enumerate(skip_c)]
        h, cin, skips = x, self._nch, []
        for k, blk in enumerate((self.inc.conv, self.down1.mpconv[1], self.down2.mpconv[1], self.down3.mpconv[1])):
            skip, h = _double(tape, h, blk, [_seg(cin)], 'enc%d' % k, out=cats[k].slice(0, cp.pad8(skip_c[k])), pool=True)
            skips.append(skip)
            cin = skip_c[k]
        h = _double(tape, h, self.down4.mpconv[1], [_seg(cin)], 'enc4')
        for k, blk in zip((3, 2, 1, 0), (self.up1, self.up2, self.up3, self.up4)):
            c = skip_c[k]
            slot = cats[k].slice(cp.pad8(c), cp.pad8(c))
            if isinstance(blk.up, nn.ConvTranspose2d):
                u = conv_unit(tape, h, blk.up.weight, blk.up.bias, [_seg(c)], stride=2, pad=0, transposed=True, act=nv.ACT_NONE,
                              bn=None, out=slot, tag='up%d.deconv' % k)
            else:
                u = upsample_nearest2x(tape, h, out=slot, tag='up%d.up' % k)
            cat = concat(tape, [(skips[k], 0), (u, cp.pad8(c))], cats[k])
            drop = None
            if k == 0:          # finaldrop (unet.py:105): Dropout2d on the last unit's output, drawn in training only
                drop = tape.dropout_table(tape.site('finaldrop'), N, cp.pad8(nf), self.finaldrop.p)
            h = _double(tape, cat, blk.conv, [_seg(c), _seg(c)], 'dec%d' % k, dropmul=drop)
        return head_1x1(tape, h, self.outc.conv.weight, self.outc.conv.bias, dlogits, tag='outc')
