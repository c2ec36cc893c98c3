"""A three-layer executor model whose convolutions are all dilated -- TEST INFRASTRUCTURE ONLY (test_dilation_cpu.py on the ABI
emulator, test_dilation_gpu.py on the device): conv3x3(3 -> 32, d = 2) -> conv3x3(32 -> 64, d = 2) -> conv3x3(64 -> 64, d = 4) + the
second layer's output, each followed by BatchNorm and ReLU, then a 1x1 classifier.  It drives ``segnb.net.conv_unit(dilation=d)``
through everything a model does with it: the activation epilogue in eval, batch statistics and the fused finalize in training,
the residual add, the backward through ``_data_gradient`` (whose fused forms must all decline) and the weight gradients.  The
channel counts and the 32 x 32 map pass the size gates of the first-layer (c8), rolling, resident-weight and LDS-DMA kernels and of
their fused BatchNorm forms, so only the span helper keeps those away.  ``reference`` is the same function in torch, float64.
"""
import torch
import torch.nn.functional as F
from torch import nn

from segnb import _native as nv
from segnb import convplan as cp
from segnb.net import HipNet, conv_unit, head_1x1

DIL = (2, 2, 4)


class DilatedNet(HipNet):
    lazy_add = True

    def __init__(self, num_classes=2):
        super(DilatedNet, self).__init__()
        self.conv1, self.bn1 = nn.Conv2d(3, 32, 3, padding=DIL[0], dilation=DIL[0], bias=False), nn.BatchNorm2d(32)
        self.conv2, self.bn2 = nn.Conv2d(32, 64, 3, padding=DIL[1], dilation=DIL[1], bias=False), nn.BatchNorm2d(64)
        self.conv3, self.bn3 = nn.Conv2d(64, 64, 3, padding=DIL[2], dilation=DIL[2], bias=False), nn.BatchNorm2d(64)
        self.head = nn.Conv2d(64, num_classes, 1)
        for i, bn in enumerate((self.bn1, self.bn2, self.bn3)):           # (non-trivial affine parameters and statistics)
            g = torch.Generator().manual_seed(40 + i)
            bn.weight.data = 0.5 + torch.rand(bn.weight.shape, generator=g)
            bn.bias.data = 0.1 * torch.randn(bn.bias.shape, generator=g)
            bn.running_mean.data = 0.1 * torch.randn(bn.bias.shape, generator=g)
            bn.running_var.data = 0.5 + torch.rand(bn.bias.shape, generator=g)
        self._init_engine(3)

    def _build(self, tape, x, dlogits):
        a = conv_unit(tape, x, self.conv1.weight, None, [(3, cp.pad8(3))], stride=1, pad=DIL[0], dilation=DIL[0], bn=self.bn1,
                      act=nv.ACT_RELU, tag='c1')
        b = conv_unit(tape, a, self.conv2.weight, None, [(32, 32)], stride=1, pad=DIL[1], dilation=DIL[1], bn=self.bn2,
                      act=nv.ACT_RELU, tag='c2')
        c = conv_unit(tape, b, self.conv3.weight, None, [(64, 64)], stride=1, pad=DIL[2], dilation=DIL[2], bn=self.bn3,
                      act=nv.ACT_RELU, res=b, tag='c3')
        return head_1x1(tape, c, self.head.weight, self.head.bias, dlogits, tag='head')


def reference(sd, x, train):
    """DilatedNet on its state_dict (any dtype); running statistics in sd advance when train"""
    def bn(p, t):
        return F.batch_norm(t, sd[p + '.running_mean'], sd[p + '.running_var'], sd[p + '.weight'], sd[p + '.bias'], training=train,
                            momentum=0.1, eps=1e-5)
    a = torch.relu(bn('bn1', F.conv2d(x, sd['conv1.weight'], None, padding=DIL[0], dilation=DIL[0])))
    b = torch.relu(bn('bn2', F.conv2d(a, sd['conv2.weight'], None, padding=DIL[1], dilation=DIL[1])))
    c = torch.relu(bn('bn3', F.conv2d(b, sd['conv3.weight'], None, padding=DIL[2], dilation=DIL[2])) + b)
    return F.conv2d(c, sd['head.weight'], sd['head.bias'])


def reference_step(model, x, G):
    """-> float64 eval logits, training logits, {name: gradient of (logits * G).sum()}, buffers after the step"""
    sd = {k: (v.detach().cpu().double().clone() if v.is_floating_point() else v.detach().cpu().clone())
          for k, v in model.state_dict().items()}
    pn = [n for n, _ in model.named_parameters()]
    with torch.no_grad():
        ev = reference({k: v.clone() for k, v in sd.items()}, x.double(), False)
    leaves = {k: (v.requires_grad_(True) if k in pn else v) for k, v in sd.items()}
    out = reference(leaves, x.double(), True)
    (out * G.double()).sum().backward()
    return ev, out.detach(), {n: leaves[n].grad for n in pn}, {k: v for k, v in leaves.items() if k not in pn}
