#!/usr/bin/env python3
"""Stand-alone times of the conv_fprop_ws_kernel launches of the ZF_UNET bs=32 224x224 step that the WsEpi instantiations serve
(segnb_tune "fprop_dma_epi": the previous tile's store rows on peeled, straight-line taps) -- 3 x 3 window, 16 x 16 or
14 x 14 tiles, 112^2 .. 14^2: forward with statistics and data gradient of encK.l1 / .l2 (= decK.l2), the virtual-concat forward
of decK.l1 and its skip-segment data gradient -- and the three plane-gather launches (data gradient of decK.l1's up segment at
56^2, 28^2 and 14^2 low resolution; below 12 columns another kernel serves it), which share the halo waves' tile switch.

    [SEGNB_LIB=<another build's libsegnb_hip.so>] python tools/wsepi_bench.py [--epi -1|0|1] [--reps 300] [--tag NAME]

One line per launch: `tag launch us` (HIP events around `reps` back-to-back launches); first the box's two calibration probes
(bench.box_calibration).  One process per knob setting, alternating A B A B inside one visit to one box (profiles/wsepi_ab.txt)."""
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
    ap.add_argument('--epi', type=int, default=-1, help='segnb_tune fprop_dma_epi (-1: the library\'s own choice; not set at all '
                                                        'where the library has no such knob: a parent build)')
    ap.add_argument('--reps', type=int, default=300)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--tag', default='run')
    ap.add_argument('--no-box', action='store_true')
    args = ap.parse_args()
    rt = Runtime('cuda', 'bf16')
    if not args.no_box:
        from bench import box_calibration
        print('%s box %s' % (args.tag, box_calibration(torch.device('cuda:0'))))
    if args.epi >= 0:
        nv.call('segnb_tune', b'fprop_dma_epi', args.epi)
    N = args.batch
    total = 0.0

    def report(name, fn):
        nonlocal total
        nv.call('segnb_tune', b'call_census', 1)
        nv.census_read()
        fn()
        served = nv.census_read().get('epi:1', 0)
        nv.call('segnb_tune', b'call_census', 0)
        us = timed(fn, args.reps)
        total += us
        print('%s %-14s %8.2f  epi:%d' % (args.tag, name, us, served), flush=True)

    for lvl, hw, c in ((1, 112, 64), (2, 56, 128), (3, 28, 256), (4, 14, 512)):
        # encK.l1: c/2 -> c (level 1: 32 input channels, another kernel), encK.l2 = decK.l2: c -> c
        for name, ci in (('enc%d.l1' % lvl, c // 2), ('enc%d.l2' % lvl, c)):
            if ci % 64:
                continue
            wt = torch.randn(c, ci, 3, 3, device='cuda') * 0.05
            op = ConvOp(rt, wt, torch.zeros(c, device='cuda'), [(ci, ci)], 1, 1, False, True)
            op.pack(hw, hw)
            xv, dyv = View.alloc(rt, N, hw, hw, ci), View.alloc(rt, N, hw, hw, c)
            xv.t.normal_()
            dyv.t.normal_()
            yv, dxv = View.alloc(rt, N, hw, hw, c), View.alloc(rt, N, hw, hw, ci)
            stats = rt.zeros((16, 2, c), torch.float64)
            report(name + '.fwd', lambda: op.fprop(xv, yv, stats))
            report(name + '.dgrad', lambda: op.dgrad(dyv, dxv))
        # decK.l1: cat([Upsample x2(u: 2c channels), skip: c channels]) -> c; virtual-concat forward, skip-segment data gradient
        cu, cs = 2 * c, c
        wt = torch.randn(c, cu + cs, 3, 3, device='cuda') * 0.05
        op = UpCatConvOp(rt, wt, torch.zeros(c, device='cuda'), [(cu, cu), (cs, cs)], need_dgrad=True)
        PackTable(rt, op.full.pack_jobs(hw, hw) + op.skip.pack_jobs(hw, hw) + op.up.pack_jobs(hw // 2, hw // 2),
                  'segnb_pack_weight_multi', 'segnb_pack_weight').run()
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
        report('dec%d.l1.vcat' % lvl, lambda: op.fprop(cat, yv, stats))
        report('dec%d.l1.skipdg' % lvl, lambda: op.skip.dgrad(dyv, skip_dx))
        if hw // 2 >= 12:       # the up segment's data gradient on the low-resolution grid: the 2 x 2-window plane gather (plain order)
            report('dec%d.l1.updg' % lvl, lambda: op.up.dgrad(dyv, duv))
        del cat, dcat
    print('%s total          %8.2f' % (args.tag, total))


if __name__ == '__main__':
    main()
