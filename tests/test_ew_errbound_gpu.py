"""The BatchNorm passes of libsegnb_hip.so on dense operands (tests/ew_dense.py) against float64 under the derived bounds of
tests/ew_oracle.py: the statistics pass, finalize + activation (and the fused forward), the backward reduction with every source
combination of tests/ew_table.py, finalize + apply (and the fused applies), on the five ew_table.SHAPES, in both dtypes, with
an ill-conditioned f32 variant (y = 100 + 0.1 randn) per shape.  Every pass starts from float64 statistics and the oracle's own
coefficients; the sums of a reduction are also checked against the float64 sums of the dz the run itself stored, and the
activations of the fused forward against the coefficients the run itself wrote.

SEGNB_RECORD_EWORACLE=1 makes a complete run add its measurements to profiles/ew_oracle_ratios.txt.
"""
import os

import pytest

import ew_dense as dn
import ew_oracle as eo
import ew_table as ew

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def record():
    rec = eo.Recorder('dense operands (tests/ew_dense.py)', dn.CASES)
    yield rec
    if os.environ.get('SEGNB_RECORD_EWORACLE') == '1':
        rec.write(eo.PROFILE)


def _from_own_coef(case, got):
    """the activations of a fused forward against the oracle's activation pass under the coefficients the run wrote"""
    _, _, (o,) = dn.parse(case)
    orc = eo.Oracle()
    mine = eo.run_backend(orc, dn.d_fwd, ew.Run(o.dt, 'cpu'), o, got['coef'].clone())
    keys = [k for k in ('out', 'pool_out', 'up_out') if k in mine]
    return eo.compare_case({k: got[k] for k in keys}, {k: mine[k] for k in keys}, orc.notes)[3]


@pytest.mark.parametrize('row', dn.ROWS)
def test_library_within_the_bound(record, row):
    failures = []
    for case in [c for c in dn.CASES if c.startswith(row + '/')]:
        orc = eo.Oracle()
        mine = eo.run_backend(orc, dn.run, case, 'cpu')
        got = {k: v.detach().cpu() for k, v in dn.run(case, ew.DEVICE).items()}
        exact, worst, left, msgs = eo.compare_case(got, mine, orc.notes)
        msgs = msgs + dn.stored_sums_failures(case, got)
        if row == 'fused' and not msgs:
            msgs = msgs + ['from its own coef: ' + m for m in _from_own_coef(case, got)]
        print(case, 'exact' if exact else 'bound', worst, left)
        failures += [(case, m) for m in msgs]
        if not msgs:
            record.add(case, exact, worst, left)
    assert not failures, failures
