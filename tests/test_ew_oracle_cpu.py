"""The emulator (oracle/abi_emulator.py) against the float64 oracle (tests/ew_oracle.py) on the 572 cases of tests/ew_table.py,
both on the CPU with the same seeds: `==` where the oracle says exact, its derived bound elsewhere; which rows are exact is
asserted; the oracle alone keeps the 1 % cap on elements left out; and every mutant -- the oracle made wrong in one way a kernel
could be wrong -- is caught by at least one case (of the table, or of tests/ew_dense.py where the table's multiples of 1/4
cannot show the defect).
"""
import pytest
import torch

import ew_dense as dn
import ew_mutants as mu
import ew_oracle as eo
import ew_table as ew
from oracle.abi_emulator import AbiEmulator

# rows that must come out exact in both dtypes (every input a small multiple of 1/4)
MUST_BE_EXACT = ('fwd', 'reduce', 'apply/', 'apply_direct/', 'stats', 'add', 'upsample/', 'nchw/', 'maxpool', 'head_fwd', 'head_bwd',
                 'head_conv', 'pack_', 'optim_sgd', 'bias_grad_multi/')
# the only rows that are not, and the operation that breaks exactness
INEXACT = {'finalize_': 'invstd = 1 / sqrt(var + eps); the unbiased running variance var * n / (n - 1)',
           'fused': 'invstd = 1 / sqrt(var + eps), and every activation through scale = gamma * invstd',
           'optim_rmsprop': 'g / (sqrt(v) + eps)',
           'optim_adam': 'the bias corrections 1 - beta^t and m / (sqrt(v / bc2) + eps)'}


def _case(case, backend):
    return eo.run_backend(backend, ew.run_outputs, case, 'cpu')


@pytest.mark.parametrize('row', sorted(ew.ROWS))
def test_emulator_matches_the_oracle(row):
    for dt in ew.row_dtypes(row):
        case = '%s:%s' % (row, dt)
        orc = eo.Oracle()
        mine = _case(case, orc)
        assert not eo.check_left_out(orc.notes), case                   # the 1 % cap, on the oracle alone
        exact, worst, left, msgs = eo.compare_case(_case(case, AbiEmulator()), mine, orc.notes)
        print(case, 'exact' if exact else 'bound', worst, left)
        assert not msgs, (case, msgs)
        assert exact == (not row.startswith(tuple(INEXACT))), (case, exact)
        if row.startswith(MUST_BE_EXACT):
            assert exact and left == 0, case


def test_the_exact_list_covers_what_it_names():
    assert all(any(r.startswith(p) for r in ew.ROWS) for p in MUST_BE_EXACT + tuple(INEXACT))
    assert not any(r.startswith(MUST_BE_EXACT) and r.startswith(tuple(INEXACT)) for r in ew.ROWS)
    assert sum(len(ew.row_dtypes(r)) for r in ew.ROWS) == len(ew.CASES) == 572


# defect -> the cases that must catch it ('dense:' cases are those of tests/ew_dense.py: on multiples of 1/4 the cancelling z is
# exact as well, and dz needs no rounding)
MUTANTS = {
    'drop_pixel': ['stats/s1:bf16', 'reduce_src1/s0:f32', 'dense:stats/s3:f32'],
    'last_max': ['reduce_src2/s1:bf16', 'maxpool3s2_scan/s0:f32', 'apply_fused_src3/s4:bf16'],
    'pool_pad_col': ['fwd_pool/s1:bf16', 'fwd_pool/s1:f32'],
    'z_cancel': ['dense:fwd/s0:f32_ill', 'dense:fwd/s3:f32_ill', 'dense:fused/s1:f32_ill'],
    'sum_before_round': ['dense:reduce_src3/s0:bf16', 'dense:reduce_src7/s2:bf16'],
    'three_taps': ['reduce_src4/s2:f32', 'apply_fused_src4/s0:bf16'],
    'drop_image0': ['fwd/s0:bf16', 'reduce_src1/s2:f32'],
    'dgamma_overwrite': ['bwd_finalize_clear/s0:f32', 'apply_fused/s1:bf16'],
}


def run_any(case, backend):
    if case.startswith('dense:'):
        return eo.run_backend(backend, dn.run, case[len('dense:'):], 'cpu')
    return _case(case, backend)


@pytest.mark.parametrize('flag', sorted(MUTANTS))
def test_mutant_is_caught(flag):
    for case in MUTANTS[flag]:
        orc = eo.Oracle()
        mine = run_any(case, orc)
        _, worst, _, msgs = eo.compare_case(run_any(case, mu.mutant(flag)), mine, orc.notes)
        print(flag, case, worst, msgs[:1])
        assert msgs, (flag, case)


# exact float64 outputs: a replicated table (as its sum), a table consumed by a finalize, a table that must be all zero
PERTURBED = [('stats/s1:f32', 'stats', 1 + 1e-9, 0.0), ('reduce_src1/s0:f32', 'sums', 1 + 1e-9, 0.0),
             ('bwd_finalize_clear/s0:f32', 'bcoef', 1 + 1e-7, 0.0), ('bwd_finalize_clear/s0:f32', 'cleared', 1.0, 1e-50),
             ('bwd_finalize_clear/s0:f32', 'sums_in', 1.0, 1e-50), ('finalize_train/s0:f32', 'nbt', 1.0, 1.0)]


@pytest.mark.parametrize('case,output,factor,plus', PERTURBED)
def test_exact_outputs_are_compared_in_their_own_precision(case, output, factor, plus):
    """`==` means float64 on the float64 tables: one element off by 1e-9 relative, or 1e-50 where zero is due, fails"""
    orc = eo.Oracle()
    mine = _case(case, orc)
    got = _case(case, AbiEmulator())
    assert not eo.compare_case(got, mine, orc.notes)[3]
    flat = got[output].view(-1)
    i = int((flat != 0).nonzero()[0]) if plus == 0.0 else 0
    before = flat[i].clone()
    flat[i] = flat[i] * factor + plus
    assert not torch.equal(flat[i], before)
    msgs = eo.compare_case(got, mine, orc.notes)[3]
    assert msgs and output in msgs[0], (case, output, msgs)
