"""The derived bounds of tests/ew_oracle.py on dense operands (tests/ew_dense.py), without a GPU: the bounds admit the emulator on
every case; the oracle alone keeps the 1 % cap on elements left out; the mutants of tests/test_ew_oracle_cpu.py fail here too;
and an fp32 implementation of the cancelling formula z = y * scale + (beta - mean * scale) exceeds the bound on the
ill-conditioned case of every shape.
"""
import pytest

import ew_dense as dn
import ew_mutants as mu
import ew_oracle as eo
from oracle.abi_emulator import AbiEmulator


def _compare(case, backend):
    orc = eo.Oracle()
    mine = eo.run_backend(orc, dn.run, case, 'cpu')
    assert not eo.check_left_out(orc.notes), case                       # the 1 % cap, on the oracle alone
    got = eo.run_backend(backend, dn.run, case, 'cpu')
    return eo.compare_case(got, mine, orc.notes) + (dn.stored_sums_failures(case, got),)


@pytest.mark.parametrize('row', dn.ROWS)
def test_bounds_admit_the_emulator(row):
    cases = [c for c in dn.CASES if c.startswith(row + '/')]
    assert len(cases) == 15
    for case in cases:
        exact, worst, left, msgs, sums = _compare(case, AbiEmulator())
        print(case, 'exact' if exact else 'bound', worst, left)
        assert not msgs and not sums, (case, msgs, sums)


# defect -> dense cases that must catch it
MUTANTS = {
    'drop_pixel': ['stats/s3:f32', 'reduce_src1/s1:bf16', 'reduce_src1_nodz/s2:f32'],
    'last_max': ['reduce_src2/s4:bf16', 'reduce_src3/s0:bf16'],      # (ties between stored bf16 activations),
    'pool_pad_col': ['fwd/s1:bf16', 'fused/s1:f32'],
    'z_cancel': ['fwd/s%d:f32_ill' % i for i in range(5)] + ['fused/s2:f32_ill'],
    'sum_before_round': ['reduce_src3/s0:bf16', 'reduce_src7/s2:bf16'],
    'three_taps': ['reduce_src4/s2:f32', 'reduce_src7/s4:bf16'],
    'drop_image0': ['fwd/s0:bf16', 'reduce_src1/s2:f32', 'apply_fused_src/s0:f32'],
    'dgamma_overwrite': ['apply/s0:f32', 'apply_fused/s1:bf16'],
}


@pytest.mark.parametrize('flag', sorted(MUTANTS))
def test_mutant_is_caught(flag):
    for case in MUTANTS[flag]:
        _, worst, _, msgs, sums = _compare(case, mu.mutant(flag))
        print(flag, case, worst, (msgs + sums)[:1])
        assert msgs or sums, (flag, case)


def test_stored_sums_check_catches_a_lost_pixel():
    """the check from the run's own dz alone (no oracle bound involved)"""
    case = 'reduce_src1/s1:f32'
    got = eo.run_backend(mu.mutant('drop_pixel'), dn.run, case, 'cpu')
    assert dn.stored_sums_failures(case, got)
    assert not dn.stored_sums_failures(case, eo.run_backend(AbiEmulator(), dn.run, case, 'cpu'))
