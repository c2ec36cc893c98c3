#!/usr/bin/env python3
"""Generate tests/golden/losses_multi.npz by running the REFERENCE's multi-class losses (lib/losses.py:105-232).

Run in the build container only (the reference is not on the GPU box):

    python tests/golden/make_golden_multiclass.py

Imports ``lib.losses`` read-only from /root/reference, as make_golden.py does, with the same repair of torch 2.x API decay:
the legacy ``size_average`` / ``reduce`` attributes that ``_Loss`` no longer stores are set on the instances, and the
undefined ``NLLLoss`` of ``NLLLAndJaccardLossMulti`` is bound to ``torch.nn.NLLLoss`` in the module's namespace.  Stores plain
arrays: per case ``<i>_x`` (fp32 input), ``<i>_t`` (int64 target), ``<i>_up`` (upstream gradient), ``<i>_loss``, ``<i>_grad``
(d(sum(loss * up))/d(x)) and ``<i>_cfg`` (JSON: class name and constructor arguments).
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference')

import numpy as np
import torch
import torch.nn.functional as F

from lib import losses as ref_losses            # reference

ref_losses.NLLLoss = torch.nn.NLLLoss            # the reference names it without importing it


def build(cfg):
    kw = dict(cfg['kw'])
    name = cfg['cls']
    if 'weight' in kw and kw['weight'] is not None:
        kw['weight'] = torch.tensor(kw['weight'], dtype=torch.float32)
    if 'class_weights' in kw and kw['class_weights'] is not None:
        kw['class_weights'] = np.array(kw['class_weights'], dtype=np.float64)
    c = getattr(ref_losses, name)(**kw)
    # torch 2.x: _Loss keeps neither size_average nor reduce
    if name == 'FocalLossMulti':
        c.size_average, c.reduce = kw.get('size_average', True), kw.get('reduce', True)
    elif name == 'JaccardLossMulti':
        c.reduce = kw.get('reduce', True)
    else:
        c.jaccard_loss.reduce = True
        if hasattr(c, 'focal_loss'):
            c.focal_loss.size_average, c.focal_loss.reduce = True, True
    return c


def main():
    g = torch.Generator().manual_seed(1234)
    cases = []
    gammas = [0, 1.5, 2, 3]
    shapes = {1: (2, 5, 8), 2: (2, 6, 7), 5: (2, 5, 8), 12: (2, 4, 6)}
    i = 0
    for C in (1, 2, 5, 12):
        N, H, W = shapes[C]
        wts = [round(0.5 + 0.25 * k, 2) for k in range(C)]
        cfgs = []
        for j, (fl, sa) in enumerate([(False, True), (True, False), (False, False), (True, True)]):
            cfgs.append({'cls': 'FocalLossMulti', 'kw': {'gamma': gammas[(j + C) % 4], 'size_average': sa, 'ignore_index': -100,
                                                       'from_logits': fl}})
        cfgs.append({'cls': 'JaccardLossMulti', 'kw': {'ignore_index': -100, 'from_logits': False, 'weight': None}})
        cfgs.append({'cls': 'JaccardLossMulti', 'kw': {'ignore_index': -100, 'from_logits': True, 'weight': wts}})
        cfgs.append({'cls': 'JaccardLossMulti', 'kw': {'ignore_index': -100, 'from_logits': False, 'weight': wts, 'reduce': False}})
        cfgs.append({'cls': 'FocalAndJaccardLossMulti', 'kw': {'jaccard_weight': 0.5, 'class_weights': None, 'ignore_index': -1}})
        cfgs.append({'cls': 'FocalAndJaccardLossMulti', 'kw': {'jaccard_weight': 2, 'class_weights': wts, 'ignore_index': -1}})
        cfgs.append({'cls': 'NLLLAndJaccardLossMulti', 'kw': {'jaccard_weight': 3, 'class_weights': None, 'ignore_index': -1}})
        cfgs.append({'cls': 'NLLLAndJaccardLossMulti', 'kw': {'jaccard_weight': 0.5, 'class_weights': wts, 'ignore_index': -1}})
        for cfg in cfgs:
            x = (2.0 * torch.randn(N, C, H, W, generator=g)).float()
            if cfg['kw'].get('from_logits'):
                x = F.log_softmax(x, dim=1)            # from_logits=True takes log-probabilities
            t = torch.randint(0, C, (N, H, W), generator=g)
            if C > 2:
                t[t == 1] = 0                          # class 1 absent from the targets
            ign = cfg['kw']['ignore_index']
            t[torch.rand(N, H, W, generator=g) < 0.15] = ign
            x = x.detach().requires_grad_(True)
            loss = build(cfg)(x, t)
            up = torch.rand(loss.shape, generator=g).float() + 0.5 if loss.dim() else torch.ones(())
            (loss * up).sum().backward()
            cases.append((i, cfg, x.detach(), t, up, loss.detach(), x.grad.detach()))
            i += 1
    out = {}
    for i, cfg, x, t, up, loss, grad in cases:
        out['%d_cfg' % i] = np.array(json.dumps(cfg))
        out['%d_x' % i] = x.numpy()
        out['%d_t' % i] = t.numpy().astype(np.int64)
        out['%d_up' % i] = up.numpy().astype(np.float32)
        out['%d_loss' % i] = loss.numpy().astype(np.float32)
        out['%d_grad' % i] = grad.numpy()
    out['n_cases'] = np.array(len(cases))
    path = os.path.join(HERE, 'losses_multi.npz')
    np.savez_compressed(path, **out)
    print('wrote %s: %d cases, %d bytes' % (path, len(cases), os.path.getsize(path)))


if __name__ == '__main__':
    main()
