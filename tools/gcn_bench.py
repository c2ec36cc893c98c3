#!/usr/bin/env python3
"""GCN34 on the MI355X: (1) train-step images/s at 512 x 512, batch 16, bf16, K = 1 (LinkNet34's row size: the two share the
encoder); (2) the decoder kernels alone (csrc/gcn.hip: every GCM / BRM / resize launch of one training step, forward and
backward) against a torch formulation of the same decoder (F.conv2d / F.interpolate with autograd, fp32) on the same GPU,
with the bytes each entry point must move and its share of the 6.3 TB/s achievable HBM rate.

    python tools/gcn_bench.py [--batch 16] [--size 512] [--classes 1] [--iters 20] [--skip-model]

Prints one JSON line per measurement.  Bytes per entry point (M = one fp32 [N, K, H, W] map, X = the encoder feature):
gcm_fwd X + 3M (feature in; yl, yr, out written), gcm_bwd 2X + 5M (feature in, its gradient out; dout, yl, yr in; dyl, dyr
out), brm_fwd 3M, brm_bwd 4M (x, r, dout in; dx out), resize fwd in + skip + out, bwd out-size in + in-size out.
"""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'segmentation-networks-benchmark_amd'), ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch
import torch.nn.functional as F

HBM = 6.3e12


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
    return ev[0].elapsed_time(ev[1]) * 1e3 / iters          # us


def model_step(B, S, K, iters):
    from lib.losses import BCEWithLogitsLossAndSmoothJaccard
    from lib.models.gcn import GCN34
    from model_checks import blob_batch
    dev = torch.device('cuda:0')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = GCN34(num_classes=K, input_size=S).to(dev).train()
    x, y = blob_batch(B, S, 1)
    x, y = x.to(dev), y.to(dev)
    opt = torch.optim.SGD(m.parameters(), lr=1e-3, momentum=0.9)
    crit = BCEWithLogitsLossAndSmoothJaccard()

    def step():
        opt.zero_grad()
        loss = crit(m(x), y)
        loss.backward()
        opt.step()
    for _ in range(5):                       # (step 3 on replays the recorded launch lists)
        step()
    us = timed(step, iters)
    return {'what': 'gcn34_train_step', 'batch': B, 'size': S, 'classes': K, 'dtype': 'bf16', 'ms_per_step': us / 1e3,
            'images_per_s': B * 1e6 / us}


class Decoder(object):
    """The decoder of one GCN34 step on fixed buffers: the same entry points, shapes and order as segnb.gcn runs them."""

    def __init__(self, B, S, K, dev):
        from segnb import _native as nv
        self.nv, self.dev, self.N, self.K = nv, dev, B, K
        self.st = torch.cuda.current_stream(dev).cuda_stream
        g = torch.Generator(device=dev).manual_seed(0)

        def rnd(*shape, s=1.0, dt=torch.float32):
            return (torch.randn(shape, generator=g, device=dev) * s).to(dt)
        self.rnd = rnd
        self.feats = [(S // 4, 64), (S // 8, 128), (S // 16, 256), (S // 32, 512)]   # fm1..fm4
        self.S0 = S // 2
        self.x = {s: rnd(B, s, s, c, dt=torch.bfloat16) for s, c in self.feats}
        self.gcm = {}
        for s, c in self.feats:
            w = [rnd(K, c, 7, 1, s=0.05), rnd(K), rnd(K, K, 1, 7, s=0.3), rnd(K), rnd(K, c, 1, 7, s=0.05), rnd(K),
                 rnd(K, K, 7, 1, s=0.3), rnd(K)]
            maps = [torch.zeros(B, K, s, s, device=dev) for _ in range(5)]       # yl yr out dyl dyr
            self.gcm[s] = (w, [torch.zeros_like(t) for t in w], maps, torch.zeros_like(self.x[s]))
        self.brm = [([rnd(K, K, 3, 3, s=0.3), rnd(K), rnd(K, K, 3, 3, s=0.3), rnd(K)]) for _ in range(9)]
        self.brm_g = [[torch.zeros_like(t) for t in w] for w in self.brm]
        self.ops = []       # (name, bytes, fn) in execution order, forward then backward

    def build(self, S_out):
        nv, P, N, K, st = self.nv, self.nv.ptr, self.N, self.K, self.st
        M = lambda s, t=None: N * K * s * (t or s) * 4
        fwd, bwd = [], []

        def gcm(s, c):
            w, gw, (yl, yr, out, dyl, dyr), dx = self.gcm[s]
            X = N * s * s * c * 2
            fwd.append(('gcm_fwd C%d %d^2' % (c, s), X + 3 * M(s), lambda: nv.call(
                'segnb_gcm_fwd', nv.BF16, P(self.x[s]), c, N, s, s, c, K, None, *[P(t) for t in w], P(yl), P(yr), P(out), st)))
            bwd.append(('gcm_bwd C%d %d^2' % (c, s), 2 * X + 5 * M(s), lambda: nv.call(
                'segnb_gcm_bwd', nv.BF16, P(self.x[s]), c, N, s, s, c, K, None, P(w[0]), P(w[2]), P(w[4]), P(w[6]), P(yl),
                P(yr), P(out), P(dyl), P(dyr), P(dx), c, *[P(t) for t in gw], st)))
            return out

        def brm(i, inp, s):
            w, gw = self.brm[i], self.brm_g[i]
            r, out, dr, dx = [torch.zeros_like(inp) for _ in range(4)]
            fwd.append(('brm_fwd %d^2' % s, 3 * M(s), lambda: nv.call(
                'segnb_brm_fwd', N, s, s, K, P(inp), P(w[0]), P(w[1]), P(w[2]), P(w[3]), P(r), P(out), st)))
            bwd.append(('brm_bwd %d^2' % s, 4 * M(s), lambda: nv.call(
                'segnb_brm_bwd', N, s, s, K, P(inp), P(w[0]), P(w[2]), P(r), P(out), P(dr), P(dx), P(gw[0]), P(gw[1]),
                P(gw[2]), P(gw[3]), st)))
            return out

        def resize(a, s_in, s_out, skip):
            out = torch.zeros(N, K, s_out, s_out, device=self.dev)
            din = torch.zeros_like(a)
            fwd.append(('resize_fwd %d->%d' % (s_in, s_out), M(s_in) + M(s_out) * (2 if skip is not None else 1), lambda: nv.call(
                'segnb_resize_bilinear_ac_fwd', N, K, s_in, s_in, P(a), s_out, s_out, P(skip), P(out), st)))
            bwd.append(('resize_bwd %d->%d' % (s_in, s_out), M(s_in) + M(s_out), lambda: nv.call(
                'segnb_resize_bilinear_ac_bwd', N, K, s_in, s_in, s_out, s_out, P(out), P(din), st)))
            return out
        (s1, c1), (s2, c2), (s3, c3), (s4, c4) = self.feats
        g1 = brm(0, gcm(s4, c4), s4)
        g2 = brm(1, gcm(s3, c3), s3)
        g3 = brm(2, gcm(s2, c2), s2)
        g4 = brm(3, gcm(s1, c1), s1)
        f1 = brm(4, resize(g1, s4, s3, g2), s3)
        f2 = brm(5, resize(f1, s3, s2, g3), s2)
        f3 = brm(6, resize(f2, s2, s1, g4), s1)
        f4 = brm(7, resize(f3, s1, self.S0, None), self.S0)
        brm(8, resize(f4, self.S0, S_out, None), S_out)
        self.ops = fwd + bwd[::-1]
        return self

    def run(self):
        for _, _, fn in self.ops:
            fn()


def torch_decoder(dec, S_out):
    """the same decoder with torch ops and autograd (fp32 NCHW features, leaf tensors: their gradients are computed too)"""
    feats = [dec.x[s].float().permute(0, 3, 1, 2).contiguous().requires_grad_(True) for s, _ in dec.feats]
    gw = [[t.clone().requires_grad_(True) for t in dec.gcm[s][0]] for s, _ in dec.feats]
    bw = [[t.clone().requires_grad_(True) for t in w] for w in dec.brm]

    def G(x, w):
        return (F.conv2d(F.conv2d(x, w[0], w[1], padding=(3, 0)), w[2], w[3], padding=(0, 3)) +
                F.conv2d(F.conv2d(x, w[4], w[5], padding=(0, 3)), w[6], w[7], padding=(3, 0)))

    def B(x, w):
        return x + F.conv2d(F.relu(F.conv2d(x, w[0], w[1], padding=1)), w[2], w[3], padding=1)

    def up(x, s):
        return F.interpolate(x, size=(s, s), mode='bilinear', align_corners=True)
    (s1, _), (s2, _), (s3, _), (s4, _) = dec.feats
    g = torch.randn(dec.N, dec.K, S_out, S_out, device=dec.dev)

    def step():
        g1, g2, g3, g4 = (B(G(feats[3], gw[3]), bw[0]), B(G(feats[2], gw[2]), bw[1]), B(G(feats[1], gw[1]), bw[2]),
                          B(G(feats[0], gw[0]), bw[3]))
        f1 = B(up(g1, s3) + g2, bw[4])
        f2 = B(up(f1, s2) + g3, bw[5])
        f3 = B(up(f2, s1) + g4, bw[6])
        f4 = B(up(f3, dec.S0), bw[7])
        out = B(up(f4, S_out), bw[8])
        out.backward(g)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--classes', type=int, default=1)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--skip-model', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    from segnb import _native as nv
    nv.load()
    if not a.skip_model:
        print(json.dumps(model_step(a.batch, a.size, a.classes, a.iters)), flush=True)
    dec = Decoder(a.batch, a.size, a.classes, dev).build(a.size)
    total_us = timed(dec.run, a.iters)
    total_bytes = sum(b for _, b, _ in dec.ops)
    torch_us = timed(torch_decoder(dec, a.size), max(3, a.iters // 4))
    print(json.dumps({'what': 'gcn_decoder_fwd_bwd', 'batch': a.batch, 'size': a.size, 'classes': a.classes,
                      'kernels_ms': total_us / 1e3, 'torch_ms': torch_us / 1e3, 'speedup': torch_us / total_us,
                      'launches': len(dec.ops), 'MB': total_bytes / 1e6, 'hbm_floor_ms': total_bytes / HBM * 1e3,
                      'hbm_pct': 100.0 * total_bytes / HBM / (total_us * 1e-6)}), flush=True)
    for name, b, fn in dec.ops:
        us = timed(fn, a.iters)
        print(json.dumps({'what': 'gcn_kernel', 'op': name, 'us': round(us, 2), 'MB': round(b / 1e6, 3),
                          'hbm_pct': round(100.0 * b / HBM / (us * 1e-6), 1)}), flush=True)


if __name__ == '__main__':
    main()
