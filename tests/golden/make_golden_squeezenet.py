#!/usr/bin/env python3
"""Generate tests/golden/squeezenet_small.npz by running the REFERENCE's SqueezeNet (lib/models/squeezenet.py:68-151).

Run in the build container only (the reference is not on the GPU box):

    python tests/golden/make_golden_squeezenet.py

Imports ``lib.models.squeezenet`` read-only from the reference checkout; the model is pure torch, so no stand-in is involved.
``F.upsample`` only warns on current torch: the warning is silenced here, nothing is patched.  Weights:
oracle.fill.seeded_state.  Two cases, each stored under its prefix:

  sq_   x 2x3x32x32: the make_golden._run_and_record recipe ((B * bce_jaccard).backward())
  ns_   x 1x3x24x40: loss = (logits * G).sum() for a seeded G; non-square, 3x5 at the bottom -- odd low-resolution extents
        under the first upsample

Per case: x, y (sq_) or G (ns_), seed, sd_keys, sd_numel, eval_logits, train_logits, the loss, gradient norms and 32 probed
entries per parameter (grad_names, grad_norms, gidx/<name>, gval/<name>).  x and G hold fp16-exact values and are stored as fp16.
"""
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as mg                         # puts the reference and the repository root on sys.path
from lib import metrics as ref_metrics           # reference
from lib.models.squeezenet import SqueezeNet     # reference
from oracle import fill


def _record(m, x, seed, y=None, G=None):
    sd = fill.seeded_state(m.state_dict(), seed)
    m.load_state_dict(sd)
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
    print('loss', float(l.detach()), 'params', sum(p.numel() for p in m.parameters()), 'logits', tuple(logits.shape))
    return out


def _randn(shape, g):
    """fp32 values that are exactly fp16 (stored as fp16: half the fixture bytes, the same numbers)"""
    return torch.randn(shape, generator=g).half().float()


def main():
    warnings.filterwarnings('ignore', message='.*upsample.*')
    out = {}
    g = torch.Generator().manual_seed(511)
    x = _randn((2, 3, 32, 32), g)
    y = (torch.rand(2, 1, 32, 32, generator=g) > 0.7).long()
    for k, v in _record(SqueezeNet(in_channels=3, num_classes=1), x, 511, y=y).items():
        out['sq_' + k] = v
    g = torch.Generator().manual_seed(513)
    x = _randn((1, 3, 24, 40), g)
    G = _randn((1, 1, 24, 40), g)
    for k, v in _record(SqueezeNet(in_channels=3, num_classes=1), x, 513, G=G).items():
        out['ns_' + k] = v
    np.savez_compressed(os.path.join(HERE, 'squeezenet_small.npz'), **out)


if __name__ == '__main__':
    main()
