"""Mutants of the float64 oracle (helper module: no fixtures, no pytest settings): each is tests/ew_oracle.py's Oracle with ONE
method overridden, wrong in one way a kernel could be wrong.  The tests run a mutant as the implementation under test and
require at least one case to fail against the unmodified oracle."""
import torch

import ew_oracle as eo
from ew_oracle import X


class DropPixel(eo.Oracle):
    """one pixel dropped from a channel sum"""
    def chan_sum(self, x):
        return eo.fsum(x[1:], 0)


class LastMax(eo.Oracle):
    """the pooled gradient (and MaxPool2d's) routed to the last maximum instead of the first"""
    @staticmethod
    def first_of(is_max, dim):
        return is_max & (is_max.flip(dim).cumsum(dim).flip(dim) == 1)


class PoolPadCol(eo.Oracle):
    """the last column of an odd width included in the last pool window of each row"""
    def pooled(self, A, H, W):
        p = eo.Oracle.pooled(self, A, H, W)
        if W % 2:
            p.v[:, :, -1] = torch.maximum(p.v[:, :, -1], A.v[:, 0:2 * (H // 2):2, W - 1])
        return p


class ZCancel(eo.Oracle):
    """an fp32 kernel that folds the mean into the shift: z = y * scale + (beta - mean * scale)"""
    def z_of(self, Y, co, res):
        if co is None:
            return eo.Oracle.z_of(self, Y, co, res)
        y32, s32, b32, m32 = (t.v.float() for t in (Y, co[0], co[1], co[2]))
        z = X((y32 * s32 + (b32 - m32 * s32)).double())
        return z if res is None else eo.add(z, res)


class SumBeforeRound(eo.Oracle):
    """dz summed before it is rounded to the storage type"""
    @staticmethod
    def summed_dz(d, D, dt):
        return X(d.v, D.e)


class ThreeTaps(eo.Oracle):
    """the four taps of the upsampled gradient reduced to three"""
    @staticmethod
    def up_taps():
        return [(0, 0), (0, 1), (1, 0)]


class DropImage0(eo.Oracle):
    """the dropout multipliers of image 0 used for every image"""
    def drop_table(self, dropmul, N, Cp):
        dm = eo.Oracle.drop_table(self, dropmul, N, Cp)
        return None if dm is None else X(dm.v[:1].expand(N, 1, 1, Cp))


class DgammaOverwrite(eo.Oracle):
    """dgamma / dbeta overwritten where they should accumulate"""
    def accumulated(self, ptr, C, new):
        return new


MUTANTS = {'drop_pixel': DropPixel, 'last_max': LastMax, 'pool_pad_col': PoolPadCol, 'z_cancel': ZCancel,
           'sum_before_round': SumBeforeRound, 'three_taps': ThreeTaps, 'drop_image0': DropImage0,
           'dgamma_overwrite': DgammaOverwrite}


def mutant(flag):
    return MUTANTS[flag]()
