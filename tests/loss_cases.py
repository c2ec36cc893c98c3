"""The case list of the loss and metric oracle tests (helper module: no fixtures, no pytest settings): one list for
tests/test_loss_oracle_gpu.py and its CPU twin, the smallest shapes that reach each path of the kernels.

Binary n against the launchers' grids (ceil(n / 1024) blocks capped at 512 for the reductions): below, at and above one block,
8 * 1024 + 5 (replica 0 of the one-launch form receives two blocks), exactly 512 blocks, a second grid-stride trip with a tail,
and 1 572 864 + 3.  Multi-class N * HW for 1, 15, 16, 17 and 33 workgroups of 256 lanes (one pixel per lane when HW % 4 != 0 or a
pointer is unaligned, four otherwise), the class-bucket edges, and one case above 1 048 576 pixels (the 1024-block cap)."""
import loss_oracle as lo

CASES = []


def _add(name, fn, **kw):
    CASES.append((name, (fn, kw)))


def run(dev, args):
    fn, kw = args
    return getattr(lo, fn)(dev, **kw)


# ---------------------------------------------------------------------------------------------------------------------- binary
for n in lo.SMALL_N:
    for align in lo.ALIGNS:
        _add('binary-pixels-%d-%s' % (n, align), 'case_binary_pixels', n=n, align=align, gammas=lo.GAMMAS)
for n, align, gammas in ((524288, 'aligned', [2.0]), (524288, 'target+1', [0.5]), (524288 + 1029, 'logits+1', [1.5]),
                         (524288 + 1029, 'dlogits+1', [0.0]), (1572864 + 3, 'aligned', [3.0, 1.0])):
    _add('binary-pixels-%d-%s' % (n, align), 'case_binary_pixels', n=n, align=align, gammas=gammas)
for spec in lo.NAMED_SPECS:
    _add('binary-reduce-8197-%s' % spec, 'case_binary_reduce', n=8 * 1024 + 5, specname=spec)
for n in lo.BINARY_N:
    if n != 8 * 1024 + 5:
        _add('binary-reduce-%d-all_norm3' % n, 'case_binary_reduce', n=n, specname='all_norm3')
for n, align in ((5, 'logits+1'), (1023, 'target+1'), (8 * 1024 + 5, 'logits+1'), (524288 + 1029, 'target+1')):
    _add('binary-reduce-%d-focal_g05-%s' % (n, align), 'case_binary_reduce', n=n, specname='focal_g05', align=align)
_add('binary-reduce-1025-bce-labels01', 'case_binary_reduce', n=1025, specname='bce', labels='01')
_add('binary-work-reuse', 'case_binary_work_reuse')
_add('binary-halves-8197', 'case_binary_halves', n=8 * 1024 + 5)
_add('binary-halves-525317', 'case_binary_halves', n=524288 + 1029)
_add('binary-degenerate', 'case_binary_degenerate')

# ---------------------------------------------------------------------------------------------------------------------- multi-class
MC_GAMMAS = [0.0, 0.5, 1.0, 2.0, 2.5, 3.0]
MC_C = [1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 256]
ALL_TERMS = dict(w_focal=1.0, w_nll=0.5, w_jaccard=1.0, norm=2.5)


def _weights(C, k):
    w = [0.5 + (i * 7 % 5) * 0.375 for i in range(C)]
    w[k % C] = 0.0
    return w


for i, C in enumerate(MC_C):
    for mode in (0, 1):
        j = i + 3 * mode
        gamma = MC_GAMMAS[j % 6]
        ign = (-1, 255, 1 if C > 2 else -1)[j % 3]
        N, HW = ((3, 37), (2, 40))[(i + mode) % 2] if C < 256 else (1, 37)
        kw = dict(ALL_TERMS, focal_mean=j % 2)
        if C > 2 and j % 2 == 0:
            kw.update(nll_weight=_weights(C, 3), jac_weight=_weights(C, 0))
        # (one class: the loss is 1 - (T + 100) / (P + 100) alone, a cancellation -- held to its closed form instead)
        _add('mc-C%d-mode%d-g%g' % (C, mode, gamma), 'case_mc', C=C, N=N, HW=HW, mode=mode, gamma=gamma, ignore_index=ign,
             degenerate=C == 1, **kw)
for wg, N, HW in ((1, 1, 37), (15, 3, 1279), (16, 3, 1365), (17, 3, 1366), (33, 3, 2731), (16, 2, 8192), (17, 2, 8196)):
    _add('mc-C5-mode0-g2-wg%d%s' % (wg, 'v' if HW % 4 == 0 else ''), 'case_mc', C=5, N=N, HW=HW, gamma=2.0, focal_mean=1,
         **ALL_TERMS)
for gamma in MC_GAMMAS:
    _add('mc-C4-mode0-g%g-lead' % gamma, 'case_mc', C=4, N=2, HW=64, gamma=gamma, data=dict(lead=True), **ALL_TERMS)
_add('mc-C33-mode0-g0.5-lead', 'case_mc', C=33, N=2, HW=61, gamma=0.5, data=dict(lead=True), **ALL_TERMS)
_add('mc-C4-mode0-g2-offset1e4', 'case_mc', C=4, N=2, HW=64, gamma=2.0, data=dict(offset=1e4), **ALL_TERMS)
_add('mc-C33-mode0-g2.5-offset1e4', 'case_mc', C=33, N=2, HW=61, gamma=2.5, data=dict(offset=1e4, lead=True), **ALL_TERMS)
_add('mc-C12-mode0-unaligned', 'case_mc', C=12, N=2, HW=64, gamma=2.0, off=1, **ALL_TERMS)
_add('mc-C9-mode1-unaligned', 'case_mc', C=9, N=2, HW=64, mode=1, gamma=1.0, off=1, **ALL_TERMS)
_add('mc-C5-reduce0', 'case_mc', C=5, N=3, HW=37, w_jaccard=1.0, reduce=0, jac_weight=_weights(5, 1))
_add('mc-C17-reduce0-mode1', 'case_mc', C=17, N=2, HW=40, mode=1, w_jaccard=1.0, reduce=0)
_add('mc-C2-1048584px', 'case_mc', C=2, N=2, HW=524292, gamma=2.0, **ALL_TERMS)
_add('mc-work-reuse', 'case_mc_work_reuse')
_add('mc-all-ignored', 'case_mc_all_ignored')

# ---------------------------------------------------------------------------------------------------------------------- metrics
HIST_SHAPES = [(1, 1), (2047, 127), (2049, 4096), (1024 * 2048 + 5, 127)]
for n, nthr in HIST_SHAPES:
    _add('hist-%d-%d' % (n, nthr), 'case_hist', n=n, nthr=nthr)
_add('hist-2049-128-two-calls', 'case_hist', n=2049, nthr=128, two_calls=True)
for n in lo.ABSMAX_N:
    _add('absmax-%d' % n, 'case_absmax', n=n)
