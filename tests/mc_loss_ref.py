"""Float64 CPU restatement of the multi-class loss ABI (include/segnb_mc_loss.h) -- TEST INFRASTRUCTURE ONLY.

``sums`` / ``finalize`` / ``backward`` restate segnb_mc_loss_reduce / _finalize / _bwd term by term; ``loss_and_grad`` chains
them; ``cfg_of`` maps a lib.losses multi-class instance to its (cfg, nll_weight, jac_weight); ``McAbiEmulator`` exposes the
entry points on raw memory the way oracle.abi_emulator.AbiEmulator does for segnb_hip.h.
"""
import torch

from oracle.abi_emulator import AbiEmulator, _mem, _geom

SMOOTH = 100.0
MODE, IGNORE, GAMMA, W_FOCAL, W_NLL, W_JAC, NORM, FOCAL_MEAN, REDUCE = range(9)


def _parts(x, t, cfg):
    x = x.double()
    C = x.shape[1]
    logp = torch.log_softmax(x, 1) if cfg[MODE] == 0 else x
    p = logp.exp()
    valid = t != cfg[IGNORE]
    inr = valid & (t >= 0) & (t < C)
    tc = torch.where(inr, t, torch.zeros_like(t))
    onehot = torch.nn.functional.one_hot(tc, C).permute(0, 3, 1, 2).double() * inr[:, None].double()
    logpt = torch.gather(logp, 1, tc[:, None])[:, 0] * inr.double()
    return C, logp, p, valid, inr, tc, onehot, logpt


def _pow(om, g):
    return torch.ones_like(om) if g == 0 else om ** g


def sums(x, t, cfg, nll_w=None):
    C, logp, p, valid, inr, tc, onehot, logpt = _parts(x, t, cfg)
    g = cfg[GAMMA]
    pt = logpt.exp()
    focal = (-_pow(1 - pt, g) * logpt)[inr].sum()
    w = nll_w.double().to(x.device)[tc] if nll_w is not None else torch.ones_like(logpt)
    out = torch.zeros(3 * C + 8, dtype=torch.float64, device=x.device)
    out[:C] = (p * onehot).sum((0, 2, 3))
    out[C:2 * C] = (p * valid[:, None].double()).sum((0, 2, 3))
    out[2 * C:3 * C] = onehot.sum((0, 2, 3))
    out[3 * C] = focal
    out[3 * C + 1] = (-w * logpt)[inr].sum()
    out[3 * C + 2] = w[inr].sum()
    out[3 * C + 3] = valid.sum()
    out[3 * C + 4] = t.numel()
    out[3 * C + 5] = (valid & ~inr).sum()
    return out


def finalize(S, C, cfg, jac_w=None):
    S = S.double()
    I, P, T = S[:C], S[C:2 * C], S[2 * C:3 * C]
    w = jac_w.double().to(S.device) if jac_w is not None else torch.ones(C, dtype=torch.float64, device=S.device)
    D = P + T - I + SMOOTH
    present = T > 0
    L = torch.where(present, 1 - (I + SMOOTH) / D, torch.zeros_like(D))
    gI = torch.where(present, -(P + T + 2 * SMOOTH) / D ** 2, torch.zeros_like(D))
    gP = torch.where(present, (I + SMOOTH) / D ** 2, torch.zeros_like(D))
    jscale = cfg[W_JAC] / cfg[NORM] if cfg[REDUCE] else 1.0
    nall, W = S[3 * C + 4], S[3 * C + 2]
    focal = S[3 * C] / nall if cfg[FOCAL_MEAN] else S[3 * C]
    nll = S[3 * C + 1] / W
    loss = cfg[W_JAC] * (w * L).sum()
    if cfg[W_FOCAL]:
        loss = loss + cfg[W_FOCAL] * focal
    if cfg[W_NLL]:
        loss = loss + cfg[W_NLL] * nll
    fin = torch.zeros(8 + 3 * C, dtype=torch.float64, device=S.device)
    fin[0] = loss / cfg[NORM]
    fin[1] = cfg[W_FOCAL] / cfg[NORM] / (nall if cfg[FOCAL_MEAN] else 1.0)
    fin[2] = cfg[W_NLL] / cfg[NORM] / W if cfg[W_NLL] else 0.0
    fin[3], fin[4], fin[5], fin[6], fin[7] = S[3 * C + 3], nall, S[3 * C + 5], focal, nll
    fin[8:8 + C] = w * L
    fin[8 + C:8 + 2 * C] = jscale * w * gI
    fin[8 + 2 * C:] = jscale * w * gP
    return fin


def backward(x, t, cfg, fin, gout, nll_w=None):
    C, logp, p, valid, inr, tc, onehot, logpt = _parts(x, t, cfg)
    fin = fin.double().to(x.device)
    gout = gout.double().to(x.device).reshape(-1)
    g0 = gout[0]
    gc = gout if not cfg[REDUCE] else g0.expand(C)
    cI = (gc * fin[8 + C:8 + 2 * C])[None, :, None, None]
    cP = (gc * fin[8 + 2 * C:])[None, :, None, None]
    g = cfg[GAMMA]
    pt = logpt.exp()
    om = 1 - pt
    dfocal = -_pow(om, g) + (0 if g == 0 else g * _pow(om, g - 1) * pt * logpt)
    w = nll_w.double().to(x.device)[tc] if nll_w is not None else torch.ones_like(logpt)
    a = (g0 * fin[1] * dfocal - g0 * fin[2] * w) * inr.double()
    gj = (cP + cI * onehot) * valid[:, None].double()
    if cfg[MODE] == 0:
        S = (p * gj).sum(1, keepdim=True)
        return a[:, None] * (onehot - p) + p * (gj - S)
    return a[:, None] * onehot + p * gj


def loss_and_grad(x, t, cfg, nll_w=None, jac_w=None, gout=None):
    """-> (loss: 0-dim or [C] per-class vector, fin, dlogits), float64"""
    C = x.shape[1]
    fin = finalize(sums(x, t, cfg, nll_w), C, cfg, jac_w)
    if gout is None:
        gout = torch.ones(1 if cfg[REDUCE] else C, dtype=torch.float64, device=x.device)
    dx = backward(x, t, cfg, fin, gout, nll_w)
    return (fin[0] if cfg[REDUCE] else fin[8:8 + C]), fin, dx


def cfg_of(mod):
    """(cfg tuple, nll weight, jaccard weight) of a lib.losses multi-class instance, as its forward passes them"""
    from segnb.mcloss import make_cfg
    name = type(mod).__name__
    if name == 'FocalLossMulti':
        return make_cfg(mode=1 if mod.from_logits else 0, ignore_index=mod.ignore_index, gamma=mod.gamma, w_focal=1.0,
                        focal_mean=1 if mod.size_average else 0), None, None
    if name == 'JaccardLossMulti':
        return make_cfg(mode=1 if mod.from_logits else 0, ignore_index=mod.ignore_index, w_jaccard=1.0,
                        reduce=1 if mod.reduce else 0), None, mod.class_weights
    if name == 'FocalAndJaccardLossMulti':
        f = mod.focal_loss
        return make_cfg(mode=0, ignore_index=f.ignore_index, gamma=f.gamma, w_focal=1.0, w_jaccard=1.0, norm=1 + mod.jaccard_weight,
                        focal_mean=1 if f.size_average else 0), None, mod.jaccard_loss.class_weights
    if name == 'NLLLAndJaccardLossMulti':
        return make_cfg(mode=0, ignore_index=mod.nll_loss.ignore_index, w_nll=1.0, w_jaccard=1.0,
                        norm=1 + mod.jaccard_weight), mod.nll_loss.weight, mod.jaccard_loss.class_weights
    raise ValueError(name)


def _spec_cfg(sp):
    return (sp.mode, sp.ignore_index, sp.gamma, sp.w_focal, sp.w_nll, sp.w_jaccard, sp.norm, sp.focal_mean, sp.reduce)


def _weights(sp, C):
    nw = _mem(sp.nll_weight, C, torch.float32).clone() if sp.nll_weight else None
    jw = _mem(sp.jac_weight, C, torch.float32).clone() if sp.jac_weight else None
    return nw, jw


class McAbiEmulator(AbiEmulator):
    """AbiEmulator + the entry points of include/segnb_mc_loss.h, on raw host memory (CPU tensors)."""

    def segnb_mc_loss_work_doubles(self, C):
        return (1024 + 64) * (3 * C + 8) + 40 if 1 <= C <= 256 else 0

    def _xt(self, logits, target, N, HW, C):
        x = _mem(logits, N * C * HW, torch.float32).view(N, C, HW, 1)
        t = _mem(target, N * HW, torch.int64).view(N, HW, 1)
        return x, t

    def segnb_mc_loss_reduce(self, logits, target, N, HW, spec, work, sums_p, stream):
        sp = _geom(spec)
        x, t = self._xt(logits, target, N, HW, sp.C)
        nw, _ = _weights(sp, sp.C)
        _mem(sums_p, 3 * sp.C + 8, torch.float64).copy_(sums(x, t, _spec_cfg(sp), nw))
        return 0

    def segnb_mc_loss_finalize(self, sums_p, spec, fin, stream):
        sp = _geom(spec)
        _, jw = _weights(sp, sp.C)
        S = _mem(sums_p, 3 * sp.C + 8, torch.float64).clone()
        _mem(fin, 8 + 3 * sp.C, torch.float32).copy_(finalize(S, sp.C, _spec_cfg(sp), jw))
        return 0

    def segnb_mc_loss_reduce_finalize(self, logits, target, N, HW, spec, work, fin, stream):
        sp = _geom(spec)
        x, t = self._xt(logits, target, N, HW, sp.C)
        nw, jw = _weights(sp, sp.C)
        cfg = _spec_cfg(sp)
        _mem(fin, 8 + 3 * sp.C, torch.float32).copy_(finalize(sums(x, t, cfg, nw), sp.C, cfg, jw))
        return 0

    def segnb_mc_loss_bwd(self, logits, target, N, HW, spec, fin, grad_out, dlogits, stream):
        sp = _geom(spec)
        C = sp.C
        x, t = self._xt(logits, target, N, HW, C)
        nw, _ = _weights(sp, C)
        F = _mem(fin, 8 + 3 * C, torch.float32).clone()
        g = _mem(grad_out, 1 if sp.reduce else C, torch.float32).clone() if grad_out else torch.ones(1)
        dx = backward(x, t, _spec_cfg(sp), F, g, nw)
        _mem(dlogits, N * C * HW, torch.float32).copy_(dx.reshape(-1))
        return 0
