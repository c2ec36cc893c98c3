#!/usr/bin/env python3
"""Stand-alone times of the conv_fprop_ws_kernel launches of the ZF_UNET bs=32 224x224 step at 56^2, 28^2 and 14^2 -- the
launches the 14 x 14-pixel tile (segnb_tune "fprop_dma_cfg" = 3) applies to: forward with statistics and data gradient of
enc2-4.l1 / .l2 and dec2-4.l2, the virtual-concat forward of dec2-4.l1 and its skip-segment data gradient.

    [SEGNB_LIB=<another build's libsegnb_hip.so>] python tools/tile14_bench.py [--cfg -1|1|3] [--reps 30] [--tag NAME]

One line per launch: `tag launch us`; first the box's two calibration probes (bench.box_calibration).  For an A/B run it once
per build and knob setting, alternating, inside one visit to one box (profiles/tile14_ab.txt)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'segmentation-networks-benchmark_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch

from segnb import _native as nv
from segnb.engine import ConvOp, PackTable, Runtime, UpCatConvOp, View


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', type=int, default=-1, help='segnb_tune fprop_dma_cfg (-1: the library\'s own choice)')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--tag', default='run')
    ap.add_argument('--no-box', action='store_true')
    ap.add_argument('--verify', action='store_true',
                    help='instead of timing: every launch under cfg 3 and under cfg 1 on the same operands -- the stored outputs must be '
                         'the same bits; prints the statistics\' worst relative difference from the float64 sums of the stored output')
    args = ap.parse_args()
    rt = Runtime('cuda', 'bf16')
    if not args.no_box:
        from bench import box_calibration
        print('%s box %s' % (args.tag, box_calibration(torch.device('cuda:0'))))
    N = args.batch
    total = 0.0

    def report(name, us):
        nonlocal total
        total += us
        print('%s %-14s %8.2f' % (args.tag, name, us), flush=True)

    def verify(name, fn, out, stats):
        """fn() under cfg 3 and cfg 1: `out` (the tensor behind the output view) bit for bit, statistics against the stored output"""
        got = {}
        for cfg in (3, 1):
            out.fill_(3.0)
            if stats is not None:
                stats.zero_()
            nv.call('segnb_tune', b'fprop_dma_cfg', cfg)
            fn()
            nv.call('segnb_tune', b'fprop_dma_cfg', -1)
            torch.cuda.synchronize()
            got[cfg] = (out.clone(), None if stats is None else stats.sum(0).clone())
        same = torch.equal(got[3][0].view(torch.int16), got[1][0].view(torch.int16))
        line = '%s %-16s outputs %s' % (args.tag, name, 'bit-equal' if same else 'DIFFER')
        if stats is not None:
            v = got[3][0].double().reshape(-1, out.shape[-1])
            for cfg in (3, 1):
                st = got[cfg][1]
                rel = max(float(((st[0] - v.sum(0)).abs() / v.abs().sum(0)).max()), float(((st[1] - (v * v).sum(0)).abs() / (v * v).sum(0)).max()))
                line += '  cfg %d statistics: worst |diff| / sum|.| %.2e' % (cfg, rel)
            line += '  cfg 3 vs cfg 1 statistics: worst |diff| / sum|.| %.2e' % float(
                ((got[3][1] - got[1][1]).abs() / torch.stack([v.abs().sum(0), (v * v).sum(0)])).max())
        print(line, flush=True)
        assert same, name

    for lvl, hw, c in ((2, 56, 128), (3, 28, 256), (4, 14, 512)):
        # encK.l1: c/2 -> c, encK.l2 = decK.l2: c -> c
        for name, ci in (('enc%d.l1' % lvl, c // 2), ('enc%d.l2' % lvl, c)):
            wt = torch.randn(c, ci, 3, 3, device='cuda') * 0.05
            op = ConvOp(rt, wt, torch.zeros(c, device='cuda'), [(ci, ci)], 1, 1, False, True)
            op.pack(hw, hw)
            xv, dyv = View.alloc(rt, N, hw, hw, ci), View.alloc(rt, N, hw, hw, c)
            xv.t.normal_()
            dyv.t.normal_()
            yv, dxv = View.alloc(rt, N, hw, hw, c), View.alloc(rt, N, hw, hw, ci)
            stats = rt.zeros((16, 2, c), torch.float64)
            if args.verify:
                verify(name + '.fwd', lambda: op.fprop(xv, yv, stats), yv.t, stats)
                verify(name + '.dgrad', lambda: op.dgrad(dyv, dxv), dxv.t, None)
                continue
            nv.call('segnb_tune', b'fprop_dma_cfg', args.cfg)
            report(name + '.fwd', timed(lambda: op.fprop(xv, yv, stats), args.reps))
            report(name + '.dgrad', timed(lambda: op.dgrad(dyv, dxv), args.reps))
            nv.call('segnb_tune', b'fprop_dma_cfg', -1)
        # decK.l1: cat([Upsample x2(u: 2c channels), skip: c channels]) -> c; virtual-concat forward, skip-segment data gradient
        cu, cs = 2 * c, c
        wt = torch.randn(c, cu + cs, 3, 3, device='cuda') * 0.05
        op = UpCatConvOp(rt, wt, torch.zeros(c, device='cuda'), [(cu, cu), (cs, cs)], need_dgrad=True)
        PackTable(rt, op.full.pack_jobs(hw, hw) + op.skip.pack_jobs(hw, hw), 'segnb_pack_weight_multi', 'segnb_pack_weight').run()
        cat, dcat = View.alloc(rt, N, hw, hw, cu + cs), View.alloc(rt, N, hw, hw, cu + cs)
        cat.t.normal_()
        uv, duv = View.alloc(rt, N, hw // 2, hw // 2, cu), View.alloc(rt, N, hw // 2, hw // 2, cu)
        uv.t.normal_()
        op.bind_up(uv, duv)
        assert op.virtual(N, hw, hw)
        dyv, yv = View.alloc(rt, N, hw, hw, c), View.alloc(rt, N, hw, hw, c)
        dyv.t.normal_()
        stats = rt.zeros((16, 2, c), torch.float64)
        skip_dx = dcat.slice(cu, cs)
        if args.verify:
            verify('dec%d.l1.vcat' % lvl, lambda: op.fprop(cat, yv, stats), yv.t, stats)
            verify('dec%d.l1.skipdg' % lvl, lambda: op.skip.dgrad(dyv, skip_dx), dcat.t, None)
            continue
        nv.call('segnb_tune', b'fprop_dma_cfg', args.cfg)
        report('dec%d.l1.vcat' % lvl, timed(lambda: op.fprop(cat, yv, stats), args.reps))
        report('dec%d.l1.skipdg' % lvl, timed(lambda: op.skip.dgrad(dyv, skip_dx), args.reps))
        nv.call('segnb_tune', b'fprop_dma_cfg', -1)
    print('%s total          %8.2f' % (args.tag, total))


if __name__ == '__main__':
    main()
