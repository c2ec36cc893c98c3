"""Mutants of the ABI emulator (helper module: no fixtures, no pytest settings): each is oracle/abi_emulator.py's AbiEmulator
wrong in ONE place, the way a fused convolution kernel could be wrong.  tests/test_conv_fused_errbound_cpu.py runs each as the
implementation under test through the checks of tests/fused_errbound.py and requires at least one of them to fail; the same
checks pass on the unmodified emulator."""
import torch

from oracle import abi_emulator as ae
from oracle.abi_emulator import _geom, _mem, _nhwc, _tdt


def _taps(gg, wp, dt):
    return _mem(wp, gg.Co * gg.ntaps * gg.Ci, dt).view(gg.Co, gg.ntaps, gg.Ci).float()


class TfPadTransformed(ae.AbiEmulator):
    """(a) the SEGNB_TF_ACT transform applied to the padding pixels too: the border sees act(BatchNorm(0)), not 0"""
    def segnb_conv_fprop_tf(self, g, dtype, in_p, tf, wp, bias, bias_n, out_p, stats, bn, stream):
        rc = ae.AbiEmulator.segnb_conv_fprop_tf(self, g, dtype, in_p, tf, wp, bias, bias_n, out_p, stats, bn, stream)
        gg, t = _geom(g), _geom(tf)
        if rc or t.kind != 1:
            return rc
        dt = _tdt(dtype)
        zero = torch.zeros(gg.N * gg.Ci, dtype=dt)
        tz = self._tf_operand(tf, zero.data_ptr(), gg.Ci, gg.N, 1, 1, gg.Ci, dtype).float().view(gg.N, 1, 1, gg.Ci)
        ring = tz.expand(gg.N, gg.Hi + 2, gg.Wi + 2, gg.Ci).clone()
        ring[:, 1:-1, 1:-1] = 0
        Wm = _taps(gg, wp, dt)
        extra = torch.zeros(gg.N, gg.Ho, gg.Wo, gg.Co)
        for k in range(gg.ntaps):
            extra += ring[:, 1 + gg.dh[k]:1 + gg.dh[k] + gg.Ho, 1 + gg.dw[k]:1 + gg.dw[k] + gg.Wo] @ Wm[:, k, :].t()
        O = _nhwc(out_p, gg.N, gg.Ho, gg.Wo, gg.Co, gg.ld_out, dt)
        O.copy_((O.float() + extra).to(dt))
        return 0


class FoldedShiftNoDrop(ae.AbiEmulator):
    """(b) the folded form act(src * (scale * drop) + (shift - mean * scale) * drop) with `drop` missing from the second constant"""
    def _tf_operand(self, tf, src, ld_src, N, H, W, C, dtype):
        t = _geom(tf)
        if t.kind != 1 or not t.drop:
            return ae.AbiEmulator._tf_operand(self, tf, src, ld_src, N, H, W, C, dtype)
        dt = _tdt(dtype)
        co = _mem(t.coef, 4 * C, torch.float32).view(4, C)
        dm = _mem(t.drop, N * C, torch.float32).view(N, 1, 1, C)
        z = _nhwc(src, N, H, W, C, ld_src, dt).float() * (co[0] * dm) + (co[1] - co[2] * co[0])
        return self._act(z, t.act, t.slope).to(dt).contiguous().view(-1)


class UpcatSeamRow(ae.AbiEmulator):
    """(c) the u pixel of high-resolution row h taken as (h + 1) >> 1 at one row seam (h = 7, next to the 8-row seam)"""
    def _upcat(self, g, dtype, in_p, src):
        g2, cat = ae.AbiEmulator._upcat(self, g, dtype, in_p, src)
        sc = _geom(src)
        cat[:, 7, :, :sc.Cu] = cat[:, 8, :, :sc.Cu]
        return g2, cat


class PhaseTapRounded(ae.AbiEmulator):
    """(d) the phase weights rounded tap by tap and then summed"""
    def _pack_masked(self, j):
        Mp, Cp, nt = int(j['Mp']), int(j['Cp']), int(j['ntaps'])
        dt = _tdt(int(j['dtype']))
        acc = torch.zeros(Mp, nt, Cp)
        for t in range(nt):
            for k in range(9):
                if int(j['tap_off'][t]) >> k & 1:
                    one = torch.zeros(Mp * Cp, dtype=torch.float32)
                    self.segnb_pack_weight(int(j['w']), one.data_ptr(), ae.F32, Mp, Cp, 1, int(j['s_m']), int(j['s_c']), [k],
                                           int(j['mmap']), int(j['cmap']), 0)
                    acc[:, t, :] += one.view(Mp, Cp).to(dt).float()
        _mem(int(j['packed']), Mp * nt * Cp, dt).view(Mp, nt, Cp).copy_(acc.to(dt))


class UpsumBf16(ae.AbiEmulator):
    """(e) the 2 x 2 window of the fused Upsample backward summed in bf16"""
    def segnb_conv_fprop_upsum(self, g, dtype, in_p, wp, out_p, dst, stream):
        rc = ae.AbiEmulator.segnb_conv_fprop_upsum(self, g, dtype, in_p, wp, out_p, dst, stream)
        gg, d = _geom(g), _geom(dst)
        dt = _tdt(dtype)
        full = torch.zeros(gg.N, gg.Ho, gg.Wo, gg.Co, dtype=dt)
        self.segnb_conv_fprop(self._regeom(gg, ld_out=gg.Co), dtype, in_p, wp, None, 0, full.data_ptr(), None, stream)
        f = full[..., :d.Cu]
        _nhwc(d.u, gg.N, gg.Ho // 2, gg.Wo // 2, d.Cu, d.ld_u, dt).copy_(
            ((f[:, 0::2, 0::2] + f[:, 0::2, 1::2]) + f[:, 1::2, 0::2]) + f[:, 1::2, 1::2])
        return rc


class ThinDropTap(ae.AbiEmulator):
    """(f) a dense layer's data gradient (8 / 16 -> >= 48 channels) without its left tap in the last column of the image"""
    def segnb_conv_fprop(self, g, dtype, in_p, wp, bias, bias_n, out_p, stats, stream):
        rc = ae.AbiEmulator.segnb_conv_fprop(self, g, dtype, in_p, wp, bias, bias_n, out_p, stats, stream)
        gg = _geom(g)
        if rc or gg.ntaps != 9 or gg.Ci not in (8, 16) or gg.Co < 48 or stats is not None:
            return rc
        dt = _tdt(dtype)
        X = _nhwc(in_p, gg.N, gg.Hi, gg.Wi, gg.Ci, gg.ld_in, dt)
        Wm = _taps(gg, wp, dt)
        k = [t for t in range(9) if gg.dh[t] == 0 and gg.dw[t] == -1][0]
        O = _nhwc(out_p, gg.N, gg.Ho, gg.Wo, gg.Co, gg.ld_out, dt)
        lost = ae._gather(X, gg, k)[:, :, -1] @ Wm[:, k, :].t()
        O[:, :, -1] = (O[:, :, -1].float() - lost).to(dt)
        return 0


class EvalBnBeforeBias(ae.AbiEmulator):
    """(g) the folded eval-mode BatchNorm applied before the bias is added instead of after it"""
    def segnb_conv_fprop_act(self, g, dtype, in_p, wp, bias, bias_n, out_p, ep, stream):
        gg, e = _geom(g), _geom(ep)
        if not e.coef:
            return ae.AbiEmulator.segnb_conv_fprop_act(self, g, dtype, in_p, wp, bias, bias_n, out_p, ep, stream)
        dt = _tdt(dtype)
        X = _nhwc(in_p, gg.N, gg.Hi, gg.Wi, gg.Ci, gg.ld_in, dt)
        O = _nhwc(out_p, gg.N, gg.Ho, gg.Wo, gg.Co, gg.ld_out, dt)
        Wm = _taps(gg, wp, dt)
        acc = torch.zeros(gg.N, gg.QH, gg.QW, gg.Co)
        for t in range(gg.ntaps):
            acc += ae._gather(X, gg, t) @ Wm[:, t, :].t()
        b = torch.zeros(gg.Co)
        if bias is not None and bias_n > 0:
            b[:bias_n] = _mem(bias, bias_n, torch.float32)
        co = _mem(e.coef, 4 * gg.Co, torch.float32).view(4, gg.Co)
        v = (acc - co[2]) * co[0] + co[1] + b
        neg = 0.0 if e.act == 1 else (float(e.slope) if e.act == 2 else 1.0)
        v = torch.where(v < 0, v * neg, v) + 0.0
        oh = torch.arange(gg.QH) * gg.out_step + gg.oh0
        ow = torch.arange(gg.QW) * gg.out_step + gg.ow0
        O[:, oh[:, None], ow[None, :], :] = v.to(dt)
        return 0


class ActGradGE(ae.AbiEmulator):
    """(h) act' taken from z >= 0: the positive side's at the kink"""
    @staticmethod
    def _actgrad(z, act, slope):
        if act == ae.ACT_RELU:
            return (z >= 0).float()
        if act == ae.ACT_LEAKY:
            return torch.where(z >= 0, torch.ones_like(z), torch.full_like(z, slope))
        return torch.ones_like(z)


MUTANTS = {'a tf_pad_transformed': TfPadTransformed, 'b folded_shift_no_drop': FoldedShiftNoDrop, 'c upcat_seam_row': UpcatSeamRow,
           'd phase_tap_rounded': PhaseTapRounded, 'e upsum_bf16': UpsumBf16, 'f thin_drop_tap': ThinDropTap,
           'g evalbn_before_bias': EvalBnBeforeBias, 'h actgrad_ge': ActGradGE}
