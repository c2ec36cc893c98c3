"""An fp32 restatement of the multi-class loss ABI and mutants of the loss emulators (helper module: no fixtures, no pytest
settings).

`LossBackend` is oracle.abi_emulator.AbiEmulator (binary losses, histogram, absmax: fp32 torch) plus the entry points of
include/segnb_mc_loss.h computed in fp32 -- an honest fp32 implementation that tests/test_loss_oracle_cpu.py holds to the bounds
of tests/loss_oracle.py.  Each mutant is that backend with ONE method overridden, wrong in one way a kernel could be wrong; the
CPU tests require every mutant to fail at least one case."""
import torch

from oracle.abi_emulator import AbiEmulator, _mem, _geom

SMOOTH = 100.0


class LossBackend(AbiEmulator):
    # ------------------------------------------------------------------ the expressions the mutants change
    @staticmethod
    def mc_masks(t, C, ignore):
        valid = t != ignore
        inr = valid & (t >= 0) & (t < C)
        return valid, inr, torch.where(inr, t, torch.zeros_like(t))

    @staticmethod
    def mc_p_mask(valid):
        return valid

    @staticmethod
    def mc_focal_count(nvalid, nall):
        return nall

    @staticmethod
    def mc_below_one(om):
        return om > 0

    @staticmethod
    def mc_logp(x, mode):
        if mode == 1:
            return x
        d = x - x.max(1, keepdim=True).values
        return d - torch.log(torch.exp(d).sum(1, keepdim=True))

    # ------------------------------------------------------------------ fp32 restatement
    def _mc_inputs(self, logits, target, N, HW, sp):
        x = _mem(logits, N * sp.C * HW, torch.float32).view(N, sp.C, HW)
        t = _mem(target, N * HW, torch.int64).view(N, HW)
        nw = _mem(sp.nll_weight, sp.C, torch.float32).clone() if sp.nll_weight else None
        return x, t, nw

    def _mc_pixel(self, x, t, sp):
        C = x.shape[1]
        logp = self.mc_logp(x, sp.mode)
        p = torch.exp(logp)
        valid, inr, tc = self.mc_masks(t, C, sp.ignore_index)
        onehot = torch.nn.functional.one_hot(tc, C).permute(0, 2, 1).bool() & inr[:, None]
        logpt = torch.gather(logp, 1, tc[:, None])[:, 0]
        return logp, p, valid, inr, tc, onehot, logpt

    @staticmethod
    def _pow(om, g):
        return torch.ones_like(om) if g == 0 else om.pow(g)

    def _mc_sums(self, x, t, sp, nw):
        C = x.shape[1]
        logp, p, valid, inr, tc, onehot, logpt = self._mc_pixel(x, t, sp)
        g = float(sp.gamma)
        om = 1 - torch.exp(logpt)
        focal = -self._pow(om, g) * logpt
        w = nw[tc] if nw is not None else torch.ones_like(logpt)
        S = torch.zeros(3 * C + 8, dtype=torch.float64)
        z = torch.zeros((), dtype=torch.float32)
        S[:C] = torch.where(onehot, p, z).double().sum((0, 2))
        S[C:2 * C] = torch.where(self.mc_p_mask(valid)[:, None], p, z).double().sum((0, 2))
        S[2 * C:3 * C] = onehot.double().sum((0, 2))
        S[3 * C] = focal[inr].double().sum()
        S[3 * C + 1] = (-w * logpt)[inr].double().sum()
        S[3 * C + 2] = w[inr].double().sum()
        S[3 * C + 3] = valid.sum()
        S[3 * C + 4] = t.numel()
        S[3 * C + 5] = (valid & ~inr).sum()
        return S

    def _mc_fin(self, S, sp):
        C = sp.C
        jw = _mem(sp.jac_weight, C, torch.float32).double() if sp.jac_weight else torch.ones(C, dtype=torch.float64)
        I, P, T = S[:C], S[C:2 * C], S[2 * C:3 * C]
        D = P + T - I + SMOOTH
        present = T > 0
        zero = torch.zeros_like(D)
        L = torch.where(present, 1 - (I + SMOOTH) / D, zero)
        gI = torch.where(present, -(P + T + 2 * SMOOTH) / D ** 2, zero)
        gP = torch.where(present, (I + SMOOTH) / D ** 2, zero)
        jscale = float(sp.w_jaccard) / float(sp.norm) if sp.reduce else 1.0
        nall, W = S[3 * C + 4], S[3 * C + 2]
        focal = S[3 * C] / self.mc_focal_count(S[3 * C + 3], nall) if sp.focal_mean else S[3 * C]
        nll = S[3 * C + 1] / W
        loss = float(sp.w_jaccard) * (jw * L).sum()
        if sp.w_focal != 0:
            loss = loss + float(sp.w_focal) * focal
        if sp.w_nll != 0:
            loss = loss + float(sp.w_nll) * nll
        fin = torch.zeros(8 + 3 * C, dtype=torch.float64)
        fin[0] = loss / float(sp.norm)
        fin[1] = float(sp.w_focal) / float(sp.norm) / (nall if sp.focal_mean else 1.0)
        fin[2] = float(sp.w_nll) / float(sp.norm) / W if sp.w_nll != 0 else 0.0
        fin[3], fin[4], fin[5], fin[6], fin[7] = S[3 * C + 3], nall, S[3 * C + 5], focal, nll
        fin[8:8 + C] = jw * L
        fin[8 + C:8 + 2 * C] = jscale * jw * gI
        fin[8 + 2 * C:] = jscale * jw * gP
        return fin.float()

    def segnb_mc_loss_work_doubles(self, C):
        return (1024 + 64) * (3 * C + 8) + 40 if 1 <= C <= 256 else 0

    def segnb_mc_loss_reduce(self, logits, target, N, HW, spec, work, sums_p, stream):
        sp = _geom(spec)
        x, t, nw = self._mc_inputs(logits, target, N, HW, sp)
        _mem(sums_p, 3 * sp.C + 8, torch.float64).copy_(self._mc_sums(x, t, sp, nw))
        return 0

    def segnb_mc_loss_finalize(self, sums_p, spec, fin, stream):
        sp = _geom(spec)
        _mem(fin, 8 + 3 * sp.C, torch.float32).copy_(self._mc_fin(_mem(sums_p, 3 * sp.C + 8, torch.float64).clone(), sp))
        return 0

    def segnb_mc_loss_reduce_finalize(self, logits, target, N, HW, spec, work, fin, stream):
        sp = _geom(spec)
        x, t, nw = self._mc_inputs(logits, target, N, HW, sp)
        _mem(fin, 8 + 3 * sp.C, torch.float32).copy_(self._mc_fin(self._mc_sums(x, t, sp, nw), sp))
        return 0

    def segnb_mc_loss_bwd(self, logits, target, N, HW, spec, fin, grad_out, dlogits, stream):
        sp = _geom(spec)
        C = sp.C
        x, t, nw = self._mc_inputs(logits, target, N, HW, sp)
        F = _mem(fin, 8 + 3 * C, torch.float32).clone()
        g = _mem(grad_out, 1 if sp.reduce else C, torch.float32).clone() if grad_out else torch.ones(1)
        logp, p, valid, inr, tc, onehot, logpt = self._mc_pixel(x, t, sp)
        gc = g if not sp.reduce else g[:1].expand(C)
        cI, cP = (gc * F[8 + C:8 + 2 * C])[None, :, None], (gc * F[8 + 2 * C:])[None, :, None]
        gam = float(sp.gamma)
        pt = torch.exp(logpt)
        om = 1 - pt
        if gam == 0:
            dfocal = -torch.ones_like(om)
        else:
            pos = self.mc_below_one(om)
            dfocal = torch.where(pos, -self._pow(om, gam) + gam * self._pow(om, gam - 1) * pt * logpt, torch.zeros_like(om))
        a = g[0] * F[1] * dfocal
        if float(F[2]) != 0:
            a = a - g[0] * F[2] * (nw[tc] if nw is not None else torch.ones_like(logpt))
        a = torch.where(inr, a, torch.zeros_like(a))[:, None]
        z = torch.zeros((), dtype=torch.float32)
        gj = torch.where(valid[:, None], cP + torch.where(onehot, cI, z), z)
        oh = onehot.float()
        if sp.mode == 0:
            dx = (a * oh - a * p) + p * (gj - (p * gj).sum(1, keepdim=True))
        else:
            dx = a * oh + p * gj
        _mem(dlogits, N * C * HW, torch.float32).copy_(dx.reshape(-1))
        return 0


# ---------------------------------------------------------------------------------------------------------------------- mutants
class DeWithoutOneMinusP(LossBackend):
    """(1 - p) dropped from de"""
    @staticmethod
    def _de(p, t):
        return p / (1 + p) - t


class GammaForGammaMinusOne(LossBackend):
    """(1 - pt)^gamma where (1 - pt)^(gamma - 1) belongs"""
    @staticmethod
    def _gm1(gamma):
        return gamma


class TailSkipped(LossBackend):
    """the n % 4 tail elements left out of the sums"""
    def segnb_seg_loss_reduce(self, logits, target, n, focal_gamma, sums, stream):
        rc = LossBackend.segnb_seg_loss_reduce(self, logits, target, n - n % 4, focal_gamma, sums, stream) if n >= 4 else 0
        _mem(sums, 8, torch.float64)[6] += n % 4 if n >= 4 else n
        return rc


class AccuracyAtHalfInclusive(LossBackend):
    """p >= 0.5 counted as above the threshold"""
    @staticmethod
    def _above_half(p):
        return p >= 0.5


class FocalMeanOverValid(LossBackend):
    """focal_mean dividing by the valid pixels instead of all pixels"""
    @staticmethod
    def mc_focal_count(nvalid, nall):
        return nvalid


class SmoothOnceInGI(LossBackend):
    """the factor 2 of `smooth` missing in GI"""
    @staticmethod
    def _gi_smooth(sm):
        return sm


class ReplicaNotSummed(LossBackend):
    """the one-launch form leaving replica 7 (the blocks 7, 15, ... of 1024 pixels) out of the total"""
    def segnb_seg_loss_reduce_finalize(self, logits, target, n, spec, work, out, stream):
        sp = _geom(spec)
        idx = torch.arange(n)
        keep = (idx // 1024) % 8 != 7
        x = _mem(logits, n, torch.float32)[keep].clone()
        t = _mem(target, n, torch.int64)[keep].clone()
        self.segnb_seg_loss_reduce(x.data_ptr(), t.data_ptr(), x.numel(), float(sp.focal_gamma), work, stream)
        _mem(work, 8, torch.float64)[6] = n
        rc = self.segnb_seg_loss_finalize(work, spec, out, stream)
        _mem(work, 128, torch.float64).zero_()
        return rc


class IgnoredInPc(LossBackend):
    """ignored pixels counted in P_c"""
    @staticmethod
    def mc_p_mask(valid):
        return torch.ones_like(valid)


class BadLabelClamped(LossBackend):
    """a bad label clamped into an index"""
    @staticmethod
    def mc_masks(t, C, ignore):
        valid = t != ignore
        return valid, valid, torch.where(valid, t.clamp(0, C - 1), torch.zeros_like(t))


class NoGuardAtPtOne(LossBackend):
    """no pt == 1 guard in the focal derivative (binary and multi-class)"""
    @staticmethod
    def _below_one(om):
        return torch.ones_like(om, dtype=torch.bool)

    @staticmethod
    def mc_below_one(om):
        return torch.ones_like(om, dtype=torch.bool)


class HistogramInclusive(LossBackend):
    """the histogram comparison th <= p instead of th < p"""
    def segnb_pr_histogram(self, logits, target, n, thresholds, nthr, hist, stream):
        p = torch.exp(torch.nn.functional.logsigmoid(_mem(logits, n, torch.float32)))
        t = _mem(target, n, torch.int64) != 0
        b = torch.bucketize(p, _mem(thresholds, nthr, torch.float32), right=True)
        H = _mem(hist, 2 * (nthr + 1), torch.int64).view(2, nthr + 1)
        H[0] += torch.bincount(b[~t], minlength=nthr + 1)
        H[1] += torch.bincount(b[t], minlength=nthr + 1)
        return 0


class AbsmaxDropsNaN(LossBackend):
    """a floating-point maximum: NaN never surfaces"""
    def segnb_absmax_f32(self, x, n, out, stream):
        a = _mem(x, n, torch.float32).abs()
        _mem(out, 1, torch.float32)[0] = torch.where(torch.isnan(a), torch.zeros_like(a), a).max()
        return 0


class LogSumExpAtFullMagnitude(LossBackend):
    """logp = x - (max + log sum): the rounding of the log-sum-exp at the logits' magnitude, not shift invariant"""
    @staticmethod
    def mc_logp(x, mode):
        if mode == 1:
            return x
        m = x.max(1, keepdim=True).values
        return x - (m + torch.log(torch.exp(x - m).sum(1, keepdim=True)))


MUTANTS = {'de_without_1mp': DeWithoutOneMinusP, 'gamma_for_gamma_minus_1': GammaForGammaMinusOne, 'tail_skipped': TailSkipped,
           'accuracy_ge_half': AccuracyAtHalfInclusive, 'focal_mean_over_valid': FocalMeanOverValid,
           'smooth_once_in_gi': SmoothOnceInGI, 'replica_not_summed': ReplicaNotSummed, 'ignored_in_pc': IgnoredInPc,
           'bad_label_clamped': BadLabelClamped, 'no_guard_at_pt_one': NoGuardAtPtOne, 'histogram_inclusive': HistogramInclusive,
           'absmax_drops_nan': AbsmaxDropsNaN, 'lse_at_full_magnitude': LogSumExpAtFullMagnitude}
