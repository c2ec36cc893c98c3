#!/usr/bin/env python3
"""What a dilated 3 x 3 layer costs on the general gather kernels, against the dense 3 x 3 of the same shape on the kernels its
shape selects (the number a specialised dilated kernel would have to beat).

    python tools/dilated_bench.py [--reps 20] [--rounds 5] [--dtype bf16] [--out profiles/dilated_ab.txt]

Shapes: the dilated layers of a ResNet101 encoder at output stride 8 -- 256 -> 256 with dilation 2 (layer3) and 512 -> 512 with
dilation 4 (layer4) -- on the H/8 maps of 224 x 224 at batch 32 (28 x 28) and 512 x 512 at batch 8 (64 x 64).  Per layer and
dilation: the forward with BatchNorm statistics, the data gradient and the weight gradient, each as the median over `rounds` of
the mean of `reps` back-to-back launches (HIP events on the launch stream, after a warm-up launch), algorithmic TFLOP/s, and the
selector that served the launch (call census).  One process, one stream, nothing beside it on the device."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'segmentation-networks-benchmark_amd'))
sys.path.insert(0, ROOT)
import torch

from segnb import _native as nv
from segnb.engine import ConvOp, Runtime, View

SHAPES = [('224^2 bs32 layer3', 32, 28, 256, 2), ('224^2 bs32 layer4', 32, 28, 512, 4),
          ('512^2 bs8  layer3', 8, 64, 256, 2), ('512^2 bs8  layer4', 8, 64, 512, 4)]


def timed(fn, reps, rounds):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps * 1e3)
    return statistics.median(out)


def served(fn):
    nv.call('segnb_tune', b'call_census', 1)
    nv.census_read()
    fn()
    torch.cuda.synchronize()
    names = [k[len('kernel:'):] for k in nv.census_read() if k.startswith('kernel:')]
    nv.call('segnb_tune', b'call_census', 0)
    return '+'.join(sorted(names)) or '?'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    rt = Runtime('cuda', args.dtype)
    lines = ['# tools/dilated_bench.py --dtype %s --reps %d --rounds %d on %s' % (args.dtype, args.reps, args.rounds,
                                                                                  torch.cuda.get_device_name(0)),
             '# us per launch (median of rounds), algorithmic TFLOP/s, serving selector; d = 1 is the dense control',
             '# %-18s %3s | %-28s | %-28s | %-28s | %s' % ('shape', 'd', 'fprop + statistics', 'dgrad', 'wgrad', 'sum us')]
    for name, N, hw, C, dil in SHAPES:
        wt = torch.randn(C, C, 3, 3, device='cuda') * (2.0 / (9 * C)) ** 0.5
        flops = 2.0 * N * hw * hw * 9 * C * C
        sums = {}
        for d in (1, dil):
            op = ConvOp(rt, wt, None, [(C, C)], 1, d, False, True, dilation=d)
            op.pack(hw, hw)
            xv, yv = View.alloc(rt, N, hw, hw, C), View.alloc(rt, N, hw, hw, C)
            dyv, dxv = View.alloc(rt, N, hw, hw, C), View.alloc(rt, N, hw, hw, C)
            xv.t.normal_()
            dyv.t.normal_()
            gw = torch.zeros_like(wt)
            stats = rt.zeros((16, 2, C), torch.float64)
            cols, tot = [], 0.0
            for fn in (lambda: op.fprop(xv, yv, stats), lambda: op.dgrad(dyv, dxv), lambda: op.wgrad(xv, dyv, gw, unpack=False)):
                us = timed(fn, args.reps, args.rounds)
                tot += us
                cols.append('%8.1f us %5.0f TF %-12s' % (us, flops / us / 1e6, served(fn)))
            sums[d] = tot
            lines.append('  %-18s %3d | %s | %s | %s | %8.1f' % ((name, d) + tuple(cols) + (tot,)))
        lines.append('  %-18s     dilated / dense: %.2f x' % (name, sums[dil] / sums[1]))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
