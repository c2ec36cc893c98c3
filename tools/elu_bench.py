#!/usr/bin/env python3
"""Stand-alone throughput of the ELU passes (csrc/elu.hip) beside the BatchNorm-layer passes that move the same bytes:
segnb_elu_fwd in place against segnb_bn_act_fwd (coef NULL, ReLU, out = y), segnb_elu_bwd with one source and one sums table
against segnb_bn_act_bwd_reduce (coef NULL, ReLU), on the same bf16 tensors in one process.  Each figure is the median of
--rounds rounds of --iters launches between two device events; the rounds alternate the two kernels, and the spread is the
range of a kernel's rounds over its median.
    python tools/elu_bench.py [--iters 50] [--rounds 7]"""
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
    for N, H, W, C in [(16, 256, 256, 128), (16, 64, 64, 512)]:
        g = torch.Generator().manual_seed(1)
        z = torch.randn((N, H, W, C), generator=g).to(torch.bfloat16).to(dev)
        gr = torch.randn((N, H, W, C), generator=g).to(torch.bfloat16).to(dev)
        y, dz = z.clone(), torch.empty_like(z)
        sums = torch.zeros((16, 2, C), dtype=torch.float64, device=dev)
        nbytes = z.numel() * 2
        runs = {
            'segnb_elu_fwd (in place)': (2 * nbytes, lambda: nv.call(
                'segnb_elu_fwd', nv.BF16, P(y), C, N, H, W, C, P(y), C, None, 0, None, 0, st)),
            'segnb_bn_act_fwd (ReLU, out = y)': (2 * nbytes, lambda: nv.call(
                'segnb_bn_act_fwd', nv.BF16, P(y), C, N, H, W, C, None, nv.ACT_RELU, 0.0, None, P(y), C, None, 0, None, 0, None, 0, st)),
            'segnb_elu_bwd (one source, sums)': (3 * nbytes, lambda: nv.call(
                'segnb_elu_bwd', nv.BF16, P(z), C, N, H, W, C, P(gr), C, None, 0, None, 0, P(dz), C, P(sums), C, None, st)),
            'segnb_bn_act_bwd_reduce (ReLU)': (3 * nbytes, lambda: nv.call(
                'segnb_bn_act_bwd_reduce', nv.BF16, P(z), C, N, H, W, C, None, nv.ACT_RELU, 0.0, None, P(gr), C, None, 0, None, 0,
                P(dz), C, P(sums), None, 0, st)),
        }
        times = {k: [] for k in runs}
        for k, (_, fn) in runs.items():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for k, (_, fn) in runs.items():
                y.copy_(z)                       # (the in-place passes start from the same values every round)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / args.iters * 1e-3)
        for k, (b, _) in runs.items():
            t = np.array(times[k])
            med = float(np.median(t))
            print(json.dumps({'shape': [N, H, W, C], 'kernel': k, 'us': round(med * 1e6, 1), 'TB_per_s': round(b / med / 1e12, 3),
                              'spread_pct': round(100 * float(t.max() - t.min()) / med, 1), 'MB_moved': round(b / 1e6, 1)}))


if __name__ == '__main__':
    main()
