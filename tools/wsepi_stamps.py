#!/usr/bin/env python3
"""Where a tile of conv_fprop_ws_kernel spends its time beyond its MFMAs: in-kernel stamps of matrix wave 0 of block 0
(segnb_tune "fprop_dma_dbg" = 32; stamp 0 tap start, 1 MFMAs issued, 2 store row issued, 3 past the tap barrier) on the C -> C
launches of the ZF_UNET bs=32 step, forward and data gradient.

    python tools/wsepi_stamps.py [--epi -1|0|1] [--reps 300]

Per launch: the stand-alone time (plain instantiation, HIP events around back-to-back launches) and its us per tap step;
then, from the stamped launch (256-row tiles: the timing instantiation exists for them only), in shader cycles:
  plain taps      mean of stamp 0 -> 1, 1 -> 2, 2 -> 3 and of the tap length over the taps that carry no store row
  row taps        the same over the taps that carry one (taps 1..8 of a tile's first chunk, from the block's second tile on)
  staging         last tap's stamp 3 -> the next tile's first stamp 0 (mean over the block's tiles)
  per tile        (row tap length - plain tap length) x 8 + staging: what a tile costs beyond its taps
  switch          the barrier wait (stamp 2 -> 3) of tap 7 in the chunks where the halo waves switch to the next tile
                  (set_fetch_tile: the chunk in front of a tile's last chunk), and of tap 7 in the other chunks
(profiles/wsepi_ab.txt, section 0)."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'segmentation-networks-benchmark_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

from segnb import _native as nv
from segnb.engine import ConvOp, Runtime, View

LAUNCHES = ((112, 64), (56, 128), (28, 256), (14, 512))


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


def stamped(fn):
    nv.call('segnb_tune', b'fprop_dma_dbg', 32)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        nv.call('segnb_tune', b'fprop_dma_dbg', 0)
    buf = (ctypes.c_ulonglong * (3 * 256 * 4))()
    nv.call('segnb_debug_stamps', ctypes.cast(buf, ctypes.c_void_p))
    return np.array(buf[:], dtype=np.uint64).reshape(3, 256, 4).astype(np.int64)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epi', type=int, default=-1, help='segnb_tune fprop_dma_epi, where the library has the knob')
    ap.add_argument('--reps', type=int, default=300)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--cus', type=int, default=256)
    ap.add_argument('--raw', default=None, help='directory for the raw stamps of every launch (.npy)')
    args = ap.parse_args()
    if args.epi >= 0:
        nv.call('segnb_tune', b'fprop_dma_epi', args.epi)
    rt = Runtime('cuda', 'bf16')
    N = args.batch
    print('launch            alone us  steps/CU  us/step | plain taps: mfma  row  barrier  length | row taps: mfma  row  barrier  length |'
          ' staging | per tile (cycles) | tap 7 barrier: switch  other')
    for hw, c in LAUNCHES:
        wt = torch.randn(c, c, 3, 3, device='cuda') * 0.05
        op = ConvOp(rt, wt, torch.zeros(c, device='cuda'), [(c, c)], 1, 1, False, True)
        op.pack(hw, hw)
        xv, dyv = View.alloc(rt, N, hw, hw, c), View.alloc(rt, N, hw, hw, c)
        xv.t.normal_()
        dyv.t.normal_()
        yv, dxv = View.alloc(rt, N, hw, hw, c), View.alloc(rt, N, hw, hw, c)
        stats = rt.zeros((16, 2, c), torch.float64)
        # the 256-row tiling of the stamped instantiation: tiles, persistent blocks per channel tile, tiles of block 0
        tiles = N * ((hw + 15) // 16) ** 2
        ntl, nch = c // 64, c // 64
        gm = min(tiles, max(1, args.cus // ntl))
        mine = (tiles + gm - 1) // gm
        nsteps = mine * nch * 9
        for what, fn in (('fwd', lambda: op.fprop(xv, yv, stats)), ('dgrad', lambda: op.dgrad(dyv, dxv))):
            # the stand-alone time under the 256-row tile too, so that it is the stamped launch's own
            nv.call('segnb_tune', b'fprop_dma_cfg', 1)
            us = timed(fn, args.reps)
            st = stamped(fn)
            nv.call('segnb_tune', b'fprop_dma_cfg', -1)
            if args.raw:
                os.makedirs(args.raw, exist_ok=True)
                np.save(os.path.join(args.raw, 'stamps_%d_%s.npy' % (hw, what)), st)
            n = min(nsteps, 255)
            plain, row, staging, switch, other7 = [], [], [], [], []
            for s in range(n):
                tile, cs = divmod(s, nch * 9)
                m = st[s]
                nxt = st[s + 1][0] - m[0] if s + 1 < nsteps and s + 1 < 256 else m[3] - m[0]
                if cs == nch * 9 - 1:       # the tile's last tap: its length ends at the barrier, the rest is the staging
                    if s + 1 < n:
                        staging.append(st[s + 1][0] - m[3])
                    nxt = m[3] - m[0]
                rec = (m[1] - m[0], m[2] - m[1], m[3] - m[2], nxt)
                if cs % 9 == 7:             # the switch stands in the chunk in front of the tile's last one (every chunk when there is one)
                    (switch if cs // 9 == max(nch - 2, 0) else other7).append(m[3] - m[2])
                (row if tile >= 1 and 1 <= cs <= 8 else plain).append(rec)
            pm = np.mean(plain, 0)
            rm = np.mean(row, 0) if row else np.zeros(4)
            sg = float(np.mean(staging)) if staging else 0.0
            per_tile = (rm[3] - pm[3]) * 8 + sg if row else sg
            print('%3d^2 %3d->%-3d %-5s %7.2f  %8d  %7.3f | %16.0f %4.0f %8.0f %7.0f | %14.0f %4.0f %8.0f %7.0f | %7.0f | %8.0f | %21.0f %6.0f' % (
                hw, c, c, what, us, nsteps, us / nsteps, pm[0], pm[1], pm[2], pm[3], rm[0], rm[1], rm[2], rm[3], sg, per_tile,
                np.mean(switch) if switch else 0.0, np.mean(other7) if other7 else 0.0), flush=True)


if __name__ == '__main__':
    main()
