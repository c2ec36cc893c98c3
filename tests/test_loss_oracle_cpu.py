"""The loss and metric oracle (tests/loss_oracle.py) on the CPU: the twin of tests/test_loss_oracle_gpu.py.

Every binary, histogram and absmax case runs through oracle/abi_emulator.py and every multi-class case through the fp32
restatement of tests/loss_mutants.py, under the very bounds the kernels are held to: an honest fp32 implementation fits them.
The ambiguity cap of the histogram and the non-vacuity of the finalize bounds are asserted here with the oracle alone, and every
mutant of tests/loss_mutants.py has to fail at least one case."""
import pytest
import torch

import loss_cases as lc
import loss_mutants as lm
import loss_oracle as lo
from segnb import _native as nv


@pytest.fixture
def backend():
    nv.set_backend_for_testing(lm.LossBackend())
    yield 'cpu'
    nv.set_backend_for_testing(None)


@pytest.mark.parametrize('name,args', lc.CASES, ids=[c[0] for c in lc.CASES])
def test_fp32_backend_fits_the_bounds(backend, name, args):
    lc.run(backend, args)


def test_histogram_ambiguity_cap_with_the_oracle_alone():
    for n, nthr in lc.HIST_SHAPES:
        x, t = lo.binary_data(n, 7, 'mixed')
        thr = torch.linspace(0, 1, max(nthr, 2), dtype=torch.float64).float()
        _, _, namb = lo.hist_oracle(x, t, thr)
        assert namb <= lo.MAX_AMBIGUOUS * n + 1, (n, nthr, namb)


def test_all_ignored_is_what_nllloss_returns():
    x = torch.randn(2, 5, 37)
    t = torch.full((2, 37), 255)
    assert bool(torch.isnan(torch.nn.NLLLoss(ignore_index=255)(torch.log_softmax(x, 1), t)))


def test_pt_one_limit_of_the_oracle():
    """pt == 1: f and df are the limit 0 for gamma > 0, with a finite bound"""
    x, t = torch.tensor([-1e4, -104.0, -40.0]), torch.zeros(3, dtype=torch.int64)
    for gamma in (0.5, 1.0, 1.5, 2.0, 3.0):
        q = lo.pix_terms(x, t, gamma)
        assert float(q['df'].v[0]) == 0.0 and float(q['f'].v[0]) == 0.0
        assert bool(torch.isfinite(q['df'].v).all()) and bool(torch.isfinite(q['df'].e).all())
        assert float(lo.out_bound(q['df']).max()) < 1e-3


MUTANT_CASES = {
    'de_without_1mp': ['binary-pixels-8197-aligned'], 'gamma_for_gamma_minus_1': ['binary-pixels-8197-aligned'],
    'tail_skipped': ['binary-reduce-5-all_norm3', 'binary-reduce-8197-all_norm3'],
    'accuracy_ge_half': ['binary-reduce-8197-bce'], 'focal_mean_over_valid': ['mc-C5-mode0-g2-wg17'],
    'smooth_once_in_gi': ['binary-reduce-8197-smooth_jaccard'], 'replica_not_summed': ['binary-reduce-8197-all_norm3'],
    'ignored_in_pc': ['mc-C5-mode0-g2-wg17'], 'bad_label_clamped': ['mc-C5-mode0-g2-wg17'],
    'no_guard_at_pt_one': ['mc-C4-mode0-g0.5-lead', 'binary-pixels-8197-aligned'],
    'histogram_inclusive': ['hist-2047-127'], 'absmax_drops_nan': ['absmax-5'],
    'lse_at_full_magnitude': ['mc-C4-mode0-g2-offset1e4'],
}


@pytest.mark.parametrize('flag', sorted(lm.MUTANTS))
def test_every_mutant_fails(flag):
    by_name = dict(lc.CASES)
    failed = []
    nv.set_backend_for_testing(lm.MUTANTS[flag]())
    try:
        for name in MUTANT_CASES[flag]:
            try:
                lc.run('cpu', by_name[name])
            except AssertionError as exc:
                failed.append((name, str(exc)[:160]))
    finally:
        nv.set_backend_for_testing(None)
    print('mutant %s fails %s' % (flag, failed))
    assert failed, 'mutant %s (%s) passes %s' % (flag, lm.MUTANTS[flag].__doc__, MUTANT_CASES[flag])
