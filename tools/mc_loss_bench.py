#!/usr/bin/env python3
"""Forward + backward time of the multi-class losses (csrc/mc_loss.hip) at 224 x 224, batch 32, against a torch
formulation of the reference's FocalAndJaccardLossMulti (log_softmax, focal through nll_loss, a per-class loop of
masked_select with a host-side emptiness test) on the same GPU, and against the HBM floor (bytes moved / 6.3 TB/s).

    python tools/mc_loss_bench.py [--classes 4 12 21 150] [--batch 32] [--size 224] [--iters 20]

Prints one JSON line per class count.  Bytes: the forward reads C * 4 + 8 bytes per pixel, the backward reads them again
and writes C * 4.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'segmentation-networks-benchmark_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch
import torch.nn.functional as F

HBM = 6.3e12


def torch_focal_jaccard(x, t, ignore_index=-1, gamma=2, jaccard_weight=1, smooth=100.0):
    """the reference's algorithm written with torch ops (what a user of the reference runs on the GPU today)"""
    logp = F.log_softmax(x, dim=1)
    logpt = -F.nll_loss(logp, t, ignore_index=ignore_index, reduction='none')
    pt = logpt.exp()
    focal = (-(1 - pt).pow(gamma) * logpt).mean()
    p = logp.exp()
    mask = t != ignore_index
    per = []
    for c in range(x.shape[1]):
        tc = torch.masked_select(t == c, mask)
        oc = torch.masked_select(p[:, c], mask)
        if int(tc.long().sum()) == 0:                 # the host sync of the reference's `if num_preds == 0`
            per.append(torch.zeros((), device=x.device))
            continue
        tf = tc.float()
        inter = (oc * tf).sum()
        union = oc.sum() + tf.sum()
        per.append(1 - (inter + smooth) / (union - inter + smooth))
    return (focal + torch.stack(per).sum()) / (1 + jaccard_weight)


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--classes', type=int, nargs='+', default=[4, 12, 21, 150])
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--iters', type=int, default=20)
    a = ap.parse_args()
    from lib.losses import FocalAndJaccardLossMulti
    from segnb import mcloss
    dev = torch.device('cuda:0')
    for C in a.classes:
        N, S = a.batch, a.size
        x = torch.randn(N, C, S, S, device=dev) * 3
        t = torch.randint(0, C, (N, S, S), device=dev)
        t[torch.rand(N, S, S, device=dev) < 0.1] = -1
        mod = FocalAndJaccardLossMulti()
        npix = N * S * S
        st = torch.cuda.current_stream(dev).cuda_stream
        holder = {}

        def fwd():
            holder['x'] = x.detach().requires_grad_(True)
            holder['loss'] = mod(holder['x'], t)

        def fwd_bwd():
            fwd()
            holder['loss'].backward()

        def ref_fwd_bwd():
            xr = x.detach().requires_grad_(True)
            torch_focal_jaccard(xr, t).backward()

        # the two passes alone, through the library (no autograd bookkeeping)
        xc, tc = x.contiguous(), t.contiguous()
        cfg = mcloss.make_cfg(mode=0, ignore_index=-1, gamma=2.0, w_focal=1.0, w_jaccard=1.0, norm=2.0, focal_mean=1)
        fin = mcloss.reduce_finalize(xc, tc, cfg, None, None)
        g = torch.ones(1, device=dev)
        dx = torch.empty_like(xc)
        cs = mcloss._cspec(C, cfg, None, None)

        def k_fwd():
            mcloss.reduce_finalize(xc, tc, cfg, None, None)

        def k_bwd():
            mcloss.nv.call('segnb_mc_loss_bwd', mcloss.nv.ptr(xc), mcloss.nv.ptr(tc), N, S * S, cs, mcloss.nv.ptr(fin),
                           mcloss.nv.ptr(g), mcloss.nv.ptr(dx), st)

        us_f = timed(k_fwd, a.iters)
        us_b = timed(k_bwd, a.iters)
        us_fb = timed(fwd_bwd, a.iters)
        us_ref = timed(ref_fwd_bwd, max(3, a.iters // 4))
        b_f = npix * (4 * C + 8)
        b_b = npix * (8 * C + 8)
        print(json.dumps({
            'classes': C, 'batch': N, 'size': S,
            'fwd_us': round(us_f, 1), 'bwd_us': round(us_b, 1), 'fwd_bwd_module_us': round(us_fb, 1),
            'torch_reference_fwd_bwd_us': round(us_ref, 1), 'speedup': round(us_ref / us_fb, 1),
            'fwd_floor_us': round(b_f / HBM * 1e6, 1), 'bwd_floor_us': round(b_b / HBM * 1e6, 1),
            'fwd_TBps': round(b_f / us_f / 1e6, 2), 'bwd_TBps': round(b_b / us_b / 1e6, 2),
            'fwd_of_peak': round(b_f / us_f / 1e6 / (HBM / 1e12), 2), 'bwd_of_peak': round(b_b / us_b / 1e6 / (HBM / 1e12), 2)}),
            flush=True)


if __name__ == '__main__':
    main()
