"""libsegnb_hip.so against the float64 oracle (tests/ew_oracle.py) on the 572 cases of tests/ew_table.py: `==` where the oracle
says exact, its derived bound elsewhere, at most 1 % of an output left out as ambiguous.  The GPU half is what
tests/test_ew_table_gpu.py runs; the oracle half runs on the CPU.

SEGNB_RECORD_EWORACLE=1 makes a complete run write its measurements to profiles/ew_oracle_ratios.txt (the thresholds stay
`==` and 1).
"""
import os

import pytest

import ew_oracle as eo
import ew_table as ew

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def record():
    rec = eo.Recorder('table (tests/ew_table.py)', ew.CASES)
    yield rec
    if os.environ.get('SEGNB_RECORD_EWORACLE') == '1':
        rec.write(eo.PROFILE)


@pytest.mark.parametrize('row', sorted(ew.ROWS))
def test_library_matches_the_oracle(record, row):
    failures = []
    for dt in ew.row_dtypes(row):
        case = '%s:%s' % (row, dt)
        orc = eo.Oracle()
        mine = eo.run_backend(orc, ew.run_outputs, case, 'cpu')
        got = {k: v.detach().cpu() for k, v in ew.run_outputs(case).items()}
        exact, worst, left, msgs = eo.compare_case(got, mine, orc.notes)
        print(case, 'exact' if exact else 'bound', worst, left)
        failures += [(case, m) for m in msgs]
        if not msgs:
            record.add(case, exact, worst, left)
    assert not failures, failures
