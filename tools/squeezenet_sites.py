#!/usr/bin/env python3
"""Which entry points and kernels serve SqueezeNet's convolutions: the call census (segnb_tune "call_census") of one eager
bf16 training step per input size.  "kernel:*" names the kernel the plain forward / weight-gradient cascades chose;
"kernel:fprop_general" / "kernel:wgrad_general" mean every specialised kernel's size gate declined the shape.
    python tools/squeezenet_sites.py [--sizes 16x1,64x2,512x16]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'segmentation-networks-benchmark_amd'))
import torch

from lib.models.squeezenet import SqueezeNet
from segnb import _native as nv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='16x1,64x2,512x16', help='comma list of SIZExBATCH')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    for item in args.sizes.split(','):
        S, B = (int(v) for v in item.split('x'))
        torch.manual_seed(0)
        m = SqueezeNet().to(dev).train()
        x = torch.randn(B, 3, S, S, device=dev)
        nv.call('segnb_tune', b'call_census', 1)
        nv.census_read()
        out = m(x)
        m._run_backward(torch.ones_like(out))          # (on this thread: the census is per thread)
        torch.cuda.synchronize()
        seen = nv.census_read()
        nv.call('segnb_tune', b'call_census', 0)
        keep = {k: v for k, v in sorted(seen.items()) if k.startswith(('kernel:', 'segnb_conv', 'segnb_elu', 'segnb_bn_act', 'segnb_add',
                                                                       'segnb_maxpool', 'segnb_head'))}
        print(json.dumps({'input': '%dx%d bs=%d' % (S, S, B), 'bottom_map': '%dx%d' % (S // 8, S // 8), 'census': keep}))
        del m


if __name__ == '__main__':
    main()
