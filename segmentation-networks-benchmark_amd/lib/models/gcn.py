"""GCN34 on the MI355X engine -- drop-in for the reference's ``lib.models.gcn152.GCN34`` (lib/models/gcn152.py:63-115):
``GCN34(num_classes, input_size, pretrained=True)``, same attribute tree / state_dict keys (``layer0.0.weight``,
``layer1.1.0.conv1.weight``, ``gcm1.conv_l1.weight``, ``brm9.conv2.bias`` ...), fp32 NCHW logits at ``input_size``.

Encoder: the ResNet34 stack LinkNet34 runs (lib.models.linknet: stem, BasicBlock x [3, 4, 6, 3]) with torchvision's
initialisation; ``pretrained=True`` warns and keeps it, as LinkNet34 does.  Decoder (segnb.gcn over csrc/gcn.hip): four
Global Convolution Modules (Dropout2d(0.1), 7x1 -> 1x7 plus 1x7 -> 7x1, C -> K = num_classes channels), nine Boundary Refine
Modules (x + conv3x3(relu(conv3x3(x)))) and align_corners=True bilinear resizes, on fp32 [N, K, H, W] maps in both compute
dtypes.  Decoder weights: kaiming_normal, zero bias (the reference's initialize_weights).
"""
import warnings

from torch import nn

from segnb import _native as nv
from segnb import convplan as cp
from segnb.gcn import boundary_refine, global_conv, resize_add
from segnb.net import HipNet, conv_unit, maxpool

from .linknet import _holder_forward, _resnet_layer, resnet_encoder


class _GlobalConvModule(nn.Module):
    """Dropout2d, then two separable 7-tap branches summed: (kh x 1 -> 1 x kw) + (1 x kw -> kh x 1)."""

    def __init__(self, in_dim, out_dim, kernel_size):
        super(_GlobalConvModule, self).__init__()
        kh, kw = kernel_size
        self.pre_drop = nn.Dropout2d(p=0.1)
        self.conv_l1 = nn.Conv2d(in_dim, out_dim, kernel_size=(kh, 1), padding=((kh - 1) // 2, 0))
        self.conv_l2 = nn.Conv2d(out_dim, out_dim, kernel_size=(1, kw), padding=(0, (kw - 1) // 2))
        self.conv_r1 = nn.Conv2d(in_dim, out_dim, kernel_size=(1, kw), padding=(0, (kw - 1) // 2))
        self.conv_r2 = nn.Conv2d(out_dim, out_dim, kernel_size=(kh, 1), padding=((kh - 1) // 2, 0))
    forward = _holder_forward


class _BoundaryRefineModule(nn.Module):
    """x + conv2(relu(conv1(x))), 3 x 3 convolutions on dim channels."""

    def __init__(self, dim):
        super(_BoundaryRefineModule, self).__init__()
        self.relu = nn.ReLU(inplace=True)
        self.conv1 = nn.Conv2d(dim, dim, kernel_size=3, padding=1)
        self.conv2 = nn.Conv2d(dim, dim, kernel_size=3, padding=1)
    forward = _holder_forward


def _size2(s):
    if isinstance(s, int):
        return (s, s)
    h, w = s
    return (int(h), int(w))


class GCN34(HipNet):
    # the encoder's stage outputs feed the next stage and a GCM: their two gradients go to the producing layer's reduction pass
    # as two sources, as in LinkNet34
    lazy_add = True

    def __init__(self, num_classes, input_size, pretrained=True):
        super(GCN34, self).__init__()
        if pretrained:
            warnings.warn('GCN34(pretrained=True): ImageNet weights cannot be downloaded here; '
                          'keeping the random initialisation (load_state_dict accepts reference checkpoints)')
        if not 1 <= num_classes <= 32:
            raise ValueError('GCN34 supports 1..32 classes (the decoder kernels, segnb_gcn_ok), got %d' % num_classes)
        self.input_size = input_size
        self.num_classes = num_classes
        self.layer0 = nn.Sequential(nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False), nn.BatchNorm2d(64),
                                    nn.ReLU(inplace=True))
        self.layer1 = nn.Sequential(nn.MaxPool2d(kernel_size=3, stride=2, padding=1), _resnet_layer(64, 64, 3, 1))
        self.layer2 = _resnet_layer(64, 128, 4, 2)
        self.layer3 = _resnet_layer(128, 256, 6, 2)
        self.layer4 = _resnet_layer(256, 512, 3, 2)
        for m in self.modules():                         # torchvision resnet initialisation
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
        self.gcm1 = _GlobalConvModule(512, num_classes, (7, 7))
        self.gcm2 = _GlobalConvModule(256, num_classes, (7, 7))
        self.gcm3 = _GlobalConvModule(128, num_classes, (7, 7))
        self.gcm4 = _GlobalConvModule(64, num_classes, (7, 7))
        for i in range(1, 10):
            setattr(self, 'brm%d' % i, _BoundaryRefineModule(num_classes))
        for name in ['gcm%d' % i for i in range(1, 5)] + ['brm%d' % i for i in range(1, 10)]:
            for m in getattr(self, name).modules():
                if isinstance(m, nn.Conv2d):
                    nn.init.kaiming_normal_(m.weight)
                    nn.init.zeros_(m.bias)
        self._init_engine(3)

    def _check_input(self, x):
        super(GCN34, self)._check_input(x)
        if x.shape[2] % 32 or x.shape[3] % 32:
            raise ValueError('GCN34 needs H and W divisible by 32, got %dx%d' % (x.shape[2], x.shape[3]))

    def _build(self, tape, x, dlogits):
        stem = conv_unit(tape, x, self.layer0[0].weight, None, [(3, cp.pad8(3))], stride=2, pad=3, bn=self.layer0[1],
                         act=nv.ACT_RELU, tag='stem')
        h = maxpool(tape, stem, 3, 2, 1, tag='stempool')
        fm1, fm2, fm3, fm4 = resnet_encoder(tape, h, (self.layer1[1], self.layer2, self.layer3, self.layer4))

        def size(a):
            return (a.v.H, a.v.W)

        gcfm1 = boundary_refine(tape, global_conv(tape, fm4, self.gcm1), self.brm1)
        gcfm2 = boundary_refine(tape, global_conv(tape, fm3, self.gcm2), self.brm2)
        gcfm3 = boundary_refine(tape, global_conv(tape, fm2, self.gcm3), self.brm3)
        gcfm4 = boundary_refine(tape, global_conv(tape, fm1, self.gcm4), self.brm4)
        fs1 = boundary_refine(tape, resize_add(tape, gcfm1, size(fm3), gcfm2), self.brm5)
        fs2 = boundary_refine(tape, resize_add(tape, fs1, size(fm2), gcfm3), self.brm6)
        fs3 = boundary_refine(tape, resize_add(tape, fs2, size(fm1), gcfm4), self.brm7)
        fs4 = boundary_refine(tape, resize_add(tape, fs3, size(stem)), self.brm8)
        return boundary_refine(tape, resize_add(tape, fs4, _size2(self.input_size)), self.brm9, dlogits)
