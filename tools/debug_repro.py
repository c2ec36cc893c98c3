#!/usr/bin/env python3
"""Which layer of the bs=32 ZF_UNET forward differs between two runs?  (per-stage conv output y and BN coefficients)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'segmentation-networks-benchmark_amd')]
import torch
from lib.models.zf_unet import ZF_UNET, ENCODER, DECODER
from oracle import train_step_ref
from segnb import _native as nv

for k, v in [a.split('=') for a in sys.argv[1:]]:
    nv.call('segnb_tune', k.encode(), int(v))
torch.manual_seed(0)
m = ZF_UNET().cuda().train()
x, y = train_step_ref.synthetic_batch(32, 224, seed=1234)
x = x.cuda()
m.dropout_override = {}
plan = None
snaps = []
for run in range(4):
    with torch.no_grad():
        out = m(x)
    torch.cuda.synchronize()
    if plan is None:
        plan = m._engine
    snap = {}
    for name in ENCODER + DECODER:
        for k, st in enumerate(plan.stages[name]):
            b = list(st._bufs.values())[0]
            snap['%s.l%d.y' % (name, k + 1)] = b['y'].t.clone()
            snap['%s.l%d.coef' % (name, k + 1)] = st.bnl.coef.clone()
    snap['logits'] = out.clone()
    snaps.append(snap)
for run in range(1, 4):
    bad = [k for k in snaps[0] if not torch.equal(snaps[0][k], snaps[run][k])]
    print('run %d vs 0: first differing: %s' % (run, bad[:4]))
    for k in bad[:2]:
        d = (snaps[0][k].float() - snaps[run][k].float()).abs()
        nz = d.nonzero()
        print('   ', k, tuple(snaps[0][k].shape), 'n diff', int((d > 0).sum()), 'max', float(d.max()), 'first idx', nz[0].tolist(), 'last idx', nz[-1].tolist())
