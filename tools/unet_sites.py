#!/usr/bin/env python3
"""Which entry points and kernels serve UNet's convolutions: the call census (segnb_tune "call_census") of one eager bf16
training step per model and input size.  "kernel:*" names the kernel the plain forward / weight-gradient cascades chose;
"kernel:fprop_general" / "kernel:wgrad_general" mean every specialised kernel's size gate declined the shape -- the shapes a
virtual-concat form of the up blocks would have to serve.
    python tools/unet_sites.py [--models unet,unet_abn,unet_deconv] [--sizes 224x32]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'segmentation-networks-benchmark_amd'))
import torch

from lib.models.unet import UNet
from lib.models.unet_abn import UNetABN
from segnb import _native as nv

MODELS = {'unet': UNet, 'unet_abn': UNetABN, 'unet_deconv': lambda: UNet(upsample=False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default='unet')
    ap.add_argument('--sizes', default='224x32', help='comma list of SIZExBATCH')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    for name in args.models.split(','):
        for item in args.sizes.split(','):
            S, B = (int(v) for v in item.split('x'))
            torch.manual_seed(0)
            m = MODELS[name]().to(dev).train()
            x = torch.randn(B, 3, S, S, device=dev)
            nv.call('segnb_tune', b'call_census', 1)
            nv.census_read()
            out = m(x)
            m._run_backward(torch.ones_like(out))          # (on this thread: the census is per thread)
            torch.cuda.synchronize()
            seen = nv.census_read()
            nv.call('segnb_tune', b'call_census', 0)
            keep = {k: v for k, v in sorted(seen.items()) if k.startswith(('kernel:', 'segnb_conv', 'segnb_upconv', 'segnb_upsample', 'segnb_bn',
                                                                           'segnb_add', 'segnb_maxpool', 'segnb_head'))}
            print(json.dumps({'model': name, 'input': '%dx%d bs=%d' % (S, S, B), 'bottom_map': '%dx%d' % (S // 16, S // 16), 'census': keep}))
            del m


if __name__ == '__main__':
    main()
