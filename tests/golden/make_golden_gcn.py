#!/usr/bin/env python3
"""Generate tests/golden/gcn34_small.npz by running the REFERENCE's GCN34 (lib/models/gcn152.py:63-115).

Run in the build container only (the reference is not on the GPU box):

    python tests/golden/make_golden_gcn.py

Imports ``lib.models.gcn152`` read-only from the reference checkout, with make_golden.py's torch.nn stand-ins for
``torchvision.models.resnet34`` (the reference's own dilated_resnet.py, dilated=False).  The four GCMs' Dropout2d is set to
p = 0.  Weights: oracle.fill.seeded_state.  Three cases, each stored under its prefix:

  k1_   K = 1, x 2x3x64x64, input_size 64: the make_golden._run_and_record recipe ((B * bce_jaccard).backward())
  k3_   K = 3, x 1x3x96x96, input_size 96: loss = (logits * G).sum() for a seeded G (isolates the model from any loss)
  rs_   K = 1, x 2x3x64x64, input_size 80: the arbitrary-ratio final resize (64 -> 80 is not a power of two)

Per case: x, y (bce cases) or G, seed, sd_keys, sd_numel, eval_logits, train_logits, the loss, gradient norms and 32 probed
entries per parameter (grad_names, grad_norms, gidx/<name>, gval/<name>), small buffers after the step (buf/<name>, k1_ only).
x and G hold fp16-exact values and are stored as fp16 (the file stays under 1 MiB).
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as mg                         # puts the reference and the repository root on sys.path
from lib import metrics as ref_metrics           # reference

mg._install_third_party_standins()
from lib.models.gcn152 import GCN34              # reference (imports the torchvision stand-in)
from oracle import fill


def _record(m, x, seed, y=None, G=None, bufs=True):
    sd = fill.seeded_state(m.state_dict(), seed)
    m.load_state_dict(sd)
    for g in (m.gcm1, m.gcm2, m.gcm3, m.gcm4):
        g.pre_drop.p = 0.0
    B = x.shape[0]
    out = {'x': x.numpy().astype(np.float16), 'seed': np.asarray(seed),
           'sd_keys': np.array(list(sd.keys())), 'sd_numel': np.array([v.numel() for v in sd.values()])}
    m.eval()
    with torch.no_grad():
        out['eval_logits'] = m(x).numpy()
    m.train()
    logits = m(x)
    out['train_logits'] = logits.detach().numpy()
    if y is not None:
        out['y'] = y.numpy()
        l = mg.ref_loss('bce_jaccard')(logits, y)
        out['loss_bce_jaccard'] = l.detach().numpy()
        out['iou'] = ref_metrics.JaccardScore()(logits.detach(), y).numpy()
        total = B * l
    else:
        out['G'] = G.numpy().astype(np.float16)
        l = (logits * G).sum()
        out['loss_dot'] = l.detach().numpy()
        total = l
    m.zero_grad()
    total.backward()
    rng = np.random.RandomState(9)
    names, norms = [], []
    for n, p in m.named_parameters():
        g = p.grad.numpy().reshape(-1)
        names.append(n)
        norms.append(np.sqrt((g.astype(np.float64) ** 2).sum()))
        gi = rng.choice(g.size, min(32, g.size), replace=False)
        out['gidx/' + n], out['gval/' + n] = gi.astype(np.int32), g[gi]
    out['grad_names'], out['grad_norms'] = np.array(names), np.array(norms)
    for n, b in m.named_buffers():
        if bufs and b.numel() <= 1024:
            out['buf/' + n] = b.numpy().copy()
    print('loss', float(l), 'params', sum(p.numel() for p in m.parameters()))
    return out


def _randn(shape, g):
    """fp32 values that are exactly fp16 (stored as fp16: half the fixture bytes, the same numbers)"""
    return torch.randn(shape, generator=g).half().float()


def main():
    out = {}
    g = torch.Generator().manual_seed(341)
    x = _randn((2, 3, 64, 64), g)
    y = (torch.rand(2, 1, 64, 64, generator=g) > 0.7).long()
    for k, v in _record(GCN34(num_classes=1, input_size=64, pretrained=False), x, 341, y=y).items():
        out['k1_' + k] = v
    g = torch.Generator().manual_seed(343)
    x = _randn((1, 3, 96, 96), g)
    G = _randn((1, 3, 96, 96), g)
    for k, v in _record(GCN34(num_classes=3, input_size=96, pretrained=False), x, 343, G=G, bufs=False).items():
        out['k3_' + k] = v
    g = torch.Generator().manual_seed(380)
    x = _randn((2, 3, 64, 64), g)
    y = (torch.rand(2, 1, 80, 80, generator=g) > 0.7).long()
    for k, v in _record(GCN34(num_classes=1, input_size=80, pretrained=False), x, 380, y=y, bufs=False).items():
        out['rs_' + k] = v
    np.savez_compressed(os.path.join(HERE, 'gcn34_small.npz'), **out)


if __name__ == '__main__':
    main()
