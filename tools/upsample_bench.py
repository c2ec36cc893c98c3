#!/usr/bin/env python3
"""Stand-alone throughput of the nearest x2 upsample passes (csrc/elementwise.hip, include/segnb_upsample.h) beside the
bilinear pair, which moves the same bytes with more arithmetic: segnb_upsample_nearest2x_fwd / _bwd against
segnb_upsample_bilinear2x_fwd / _bwd on the same bf16 tensors in one process (shapes: the LOW-resolution tensor).  Each figure
is the median of --rounds rounds of --iters launches between two device events; the rounds alternate the kernels, and the
spread is the range of a kernel's rounds over its median.  A nearest kernel is expected to be no slower than its bilinear
counterpart by more than the larger of the two spreads; the last line per shape says whether that held.
    python tools/upsample_bench.py [--iters 50] [--rounds 7]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'segmentation-networks-benchmark_amd'))
import numpy as np
import torch

from segnb import _native as nv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream(dev).cuda_stream
    P = nv.ptr
    for N, H, W, C in [(16, 128, 128, 128), (16, 32, 32, 512)]:
        g = torch.Generator().manual_seed(1)
        x = torch.randn((N, H, W, C), generator=g).to(torch.bfloat16).to(dev)
        go = torch.randn((N, 2 * H, 2 * W, C), generator=g).to(torch.bfloat16).to(dev)
        out, dx = torch.empty_like(go), torch.empty_like(x)
        nbytes = 5 * x.numel() * 2                      # one low-resolution tensor and one four times its size, either direction
        runs = {}
        for kind in ('nearest', 'bilinear'):
            runs['segnb_upsample_%s2x_fwd' % kind] = (lambda k=kind: nv.call(
                'segnb_upsample_%s2x_fwd' % k, nv.BF16, P(x), C, N, H, W, C, P(out), C, st))
            runs['segnb_upsample_%s2x_bwd' % kind] = (lambda k=kind: nv.call(
                'segnb_upsample_%s2x_bwd' % k, nv.BF16, P(go), C, N, H, W, C, P(dx), C, st))
        times = {k: [] for k in runs}
        for fn in runs.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for k, fn in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / args.iters * 1e-3)
        med, spread = {}, {}
        for k in runs:
            t = np.array(times[k])
            med[k] = float(np.median(t))
            spread[k] = float(t.max() - t.min()) / med[k]
            print(json.dumps({'shape': [N, H, W, C], 'kernel': k, 'us': round(med[k] * 1e6, 1), 'TB_per_s': round(nbytes / med[k] / 1e12, 3),
                              'spread_pct': round(100 * spread[k], 1), 'MB_moved': round(nbytes / 1e6, 1)}))
        for d in ('fwd', 'bwd'):
            a, b = 'segnb_upsample_nearest2x_' + d, 'segnb_upsample_bilinear2x_' + d
            slack = max(spread[a], spread[b])
            print(json.dumps({'shape': [N, H, W, C], 'direction': d, 'nearest_over_bilinear': round(med[a] / med[b], 3),
                              'allowed': round(1.0 + slack, 3), 'held': bool(med[a] <= med[b] * (1.0 + slack))}))


if __name__ == '__main__':
    main()
