#!/usr/bin/env python3
"""Generate tests/golden/unet_small.npz by running the REFERENCE's UNet and UNetABN (lib/models/unet.py:80-107,
lib/models/unet_abn.py:80-107).

Run where make_golden.py runs (it needs the reference checkout):

    python tests/golden/make_golden_unet.py

Imports ``lib.models.unet`` and ``lib.models.unet_abn`` read-only from the reference checkout.  UNet is pure torch; UNetABN
takes ``lib.modules.abn.InPlaceABN`` from make_golden's stand-in (BatchNorm2d semantics + LeakyReLU(0.01): the un-vendored
``inplace_abn`` backend restated from its published definition, as for linknet_small.npz).  ``n_filters=8``,
``finaldrop.p = 0``, weights: oracle.fill.seeded_state.  Five cases, each stored under its prefix:

  sq_   UNet()                  x 2x3x32x32   seed 612
  ns_   UNet()                  x 1x3x32x48   seed 613    non-square, one image
  dc_   UNet(upsample=False)    x 2x3x32x32   seed 617    the ConvTranspose2d(C, C, 2, stride=2) branch
  g1_   UNet(n_channels=1)      x 2x1x32x32   seed 619    Afterburner's network
  abn_  UNetABN()               x 2x3x32x32   seed 622

32 pixels is the smallest side that leaves a 2x2 bottom map (BatchNorm over the two values of a 1x1 map is degenerate).

Per case: x, y, seed, sd_keys, sd_numel, eval_logits, train_logits, loss_bce_jaccard ((B * bce_jaccard).backward()), iou,
gradient norms and 32 probed entries per parameter (grad_names, grad_norms, gidx/<name>, gval/<name>), buffers of at most 1024
elements after the training forward (buf/<name>).  x holds fp16-exact values and is stored as fp16.

The seeds are a condition: the tests compare the fixture with check_product_golden's fp32 tolerances (logits 2e-4 of their
scale, loss 1e-5, gradient norms 1e-2, probes 5e-2 of the tensor's scale), so the reference's own fp32 values must sit well
inside them.  Per case the reference is also run in float64 on the same weights and batch, and the generator FAILS unless every
fp32-vs-float64 difference is at most a tenth of its bound (seed 611 for sq_ gives 5.7e-3 on a gradient norm and 621 for abn_
1.6e-2 -- a pre-activation or pooling tie -- and are not used).
"""
import copy
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as mg                         # puts the reference and the repository root on sys.path
from lib import metrics as ref_metrics           # reference
from oracle import fill, losses_ref

CASES = [                                        # prefix, model, constructor arguments, x shape, seed
    ('sq_', 'UNet', {}, (2, 3, 32, 32), 612),
    ('ns_', 'UNet', {}, (1, 3, 32, 48), 613),
    ('dc_', 'UNet', {'upsample': False}, (2, 3, 32, 32), 617),
    ('g1_', 'UNet', {'n_channels': 1}, (2, 1, 32, 32), 619),
    ('abn_', 'UNetABN', {}, (2, 3, 32, 32), 622),
]
# check_product_golden's fp32 bounds (tests/model_checks.py)
LOGIT_RTOL, LOSS_ATOL, NORM_RTOL, PROBE_RTOL = 2e-4, 1e-5, 1e-2, 5e-2


def _float64_run(m, x, y):
    """the same module in float64 -> (eval logits, train logits, loss, {name: gradient})"""
    m64 = copy.deepcopy(m).double()
    m64.eval()
    with torch.no_grad():
        ev = m64(x.double())
    m64.train()
    logits = m64(x.double())
    l = losses_ref.bce_jaccard(logits, y)
    m64.zero_grad()
    (x.shape[0] * l).backward()
    return ev, logits.detach(), float(l), {n: p.grad.reshape(-1) for n, p in m64.named_parameters()}


def _conditioning(tag, out, m, ref64):
    """the reference in fp32 against itself in float64, as fractions of check_product_golden's bounds; fails above a tenth"""
    ev64, tr64, l64, g64 = ref64
    worst = {}
    worst['eval logits'] = float(np.abs(out['eval_logits'] - ev64.numpy()).max() / (LOGIT_RTOL * np.abs(out['eval_logits']).max()))
    worst['train logits'] = float(np.abs(out['train_logits'] - tr64.numpy()).max() / (LOGIT_RTOL * np.abs(out['train_logits']).max()))
    worst['loss'] = abs(float(out['loss_bce_jaccard']) - l64) / LOSS_ATOL
    norms = dict(zip(out['grad_names'], out['grad_norms']))
    gmax = max(norms.values())
    wn = wp = wrel = 0.0
    for n, _ in m.named_parameters():
        if norms[n] < 1e-6 * gmax:
            continue                                  # analytically zero (a convolution bias in front of a normalisation)
        g = g64[n]
        n64 = float(g.norm())
        wrel = max(wrel, abs(n64 - norms[n]) / n64)
        wn = max(wn, abs(n64 - norms[n]) / (NORM_RTOL * norms[n]))
        ref = out['gval/' + n].astype(np.float64)
        scale = max(np.abs(ref).max(), norms[n] / np.sqrt(g.numel()))
        wp = max(wp, float(np.abs(g.numpy()[out['gidx/' + n]] - ref).max() / (PROBE_RTOL * scale)))
    worst['gradient norms'], worst['gradient probes'] = wn, wp
    print('%s fp32 vs float64, as a fraction of the bound: %s; worst relative norm difference %.2e'
          % (tag, ', '.join('%s %.3f' % kv for kv in worst.items()), wrel))
    bad = {k: v for k, v in worst.items() if not v <= 0.1}
    assert not bad, '%s: the reference in fp32 is more than a tenth of the bound from float64 (choose another seed): %s' % (tag, bad)


def _record(m, x, y, seed, tag):
    sd = fill.seeded_state(m.state_dict(), seed)
    m.load_state_dict(sd)
    m.finaldrop.p = 0.0
    ref64 = _float64_run(m, x, y)                 # (before the fp32 training forward moves the running statistics)
    B = x.shape[0]
    out = {'x': x.numpy().astype(np.float16), 'y': y.numpy(), 'seed': np.asarray(seed),
           'sd_keys': np.array(list(sd.keys())), 'sd_numel': np.array([v.numel() for v in sd.values()])}
    m.eval()
    with torch.no_grad():
        out['eval_logits'] = m(x).numpy()
    m.train()
    logits = m(x)
    out['train_logits'] = logits.detach().numpy()
    l = mg.ref_loss('bce_jaccard')(logits, y)
    out['loss_bce_jaccard'] = l.detach().numpy()
    out['iou'] = ref_metrics.JaccardScore()(logits.detach(), y).numpy()
    m.zero_grad()
    (B * l).backward()
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
        if b.numel() <= 1024:
            out['buf/' + n] = b.numpy().copy()
    print('%s loss %.6f params %d logits %s' % (tag, float(l.detach()), sum(p.numel() for p in m.parameters()), tuple(logits.shape)))
    _conditioning(tag, out, m, ref64)
    return out


def _randn(shape, g):
    """fp32 values that are exactly fp16 (stored as fp16: half the fixture bytes, the same numbers)"""
    return torch.randn(shape, generator=g).half().float()


def main():
    from lib.models.unet import UNet                  # reference
    mg._install_third_party_standins()                # lib.modules.abn.InPlaceABN, before the reference's unet_abn binds it
    from lib.models.unet_abn import UNetABN           # reference
    classes = {'UNet': UNet, 'UNetABN': UNetABN}
    out = {}
    for prefix, name, kw, shape, seed in CASES:
        g = torch.Generator().manual_seed(seed)
        x = _randn(shape, g)
        y = (torch.rand((shape[0], 1) + shape[2:], generator=g) > 0.7).long()
        for k, v in _record(classes[name](n_filters=8, **kw), x, y, seed, prefix).items():
            out[prefix + k] = v
    np.savez_compressed(os.path.join(HERE, 'unet_small.npz'), **out)


if __name__ == '__main__':
    main()
