"""The host side of the convolution entry points (csrc/conv_igemm.hip) against a table recorded on the commit before its helpers
were factored out (tests/conv_select_parent.json, written by tests/conv_select.py on that commit; never by the code under test):

  1. which kernel serves the forward, data gradient and weight gradient of small geometries that between them reach every
     selector of the two plain cascades (those that no small geometry reaches: conv_select.UNREACHED, with the gate);
  2. the answer of every fast-path query over a grid of geometries -- host functions, so this one runs without a GPU too;
  3. SHA-256 of the output bytes of every launch of 1: the kernels and their arguments did not change, so neither do the bits
     (left out: weight gradients of the general kernel, which sums with fp32 atomics -- named in the table);
  4. status and message of the refusals that moved into helpers, and which call consumes an armed segnb_wgrad_target;
  5. SHA-256 of every stored tensor of the fused entry points at their smallest served shapes (conv_select.fused_table: the drivers
     of tests/fused_errbound.py and three ConvOp launches); a sum table the parent does not repeat is named in its row.
"""
import json
import os

import pytest

import conv_select as cs
from segnb import _native as nv

with open(cs.JSON_PATH) as f:
    PARENT = json.load(f)

gpu = pytest.mark.gpu


def test_table_covers_every_selector():
    seen = {n for c in PARENT['cases'].values() for side in c['names'] for n in side}
    assert sorted(PARENT['cases']) == sorted(cs.CASES)
    assert seen | set(cs.UNREACHED) == set(cs.FPROP_SELECTORS + cs.WGRAD_SELECTORS)
    assert not seen & set(cs.UNREACHED)
    for k, c in PARENT['cases'].items():
        assert c['y'] and c['dx'], k                                   # no forward or data-gradient row is left out
        assert c['dW'] or ('kernel:wgrad_general' in c['names'][2] and c['dW_excluded'] == cs.DW_EXCLUDED), k


def test_fused_section_leaves_no_stored_tensor_out():
    rows = PARENT['fused']
    assert len(rows) == 12 and sum(not r.get('served', True) for r in rows.values()) == 1      # (the transposed case with BatchNorm)
    for k, row in rows.items():
        left_out = [t for t, v in row.items() if v is None]
        assert set(left_out) <= set(cs.FUSED_SUM_TABLES), (k, left_out)          # no forward or data-gradient tensor is left out
        assert not left_out or row['excluded'] == cs.FUSED_EXCLUDED, k
        assert row.get('served', True) is False or any(t in row for t in ('y', 'dx', 'y plain')), k


@gpu
def test_fused_outputs_are_bit_identical_to_the_parents():
    got = cs.fused_table()
    assert sorted(got) == sorted(PARENT['fused'])
    for k, want in sorted(PARENT['fused'].items()):
        assert sorted(got[k]) == sorted(t for t in want if t != 'excluded'), k
        for t, v in want.items():
            if v is not None and t != 'excluded':
                assert got[k][t] == v, (k, t)


@pytest.fixture(scope='module')
def ran():
    """every case once: {id: run_case()}"""
    return {k: cs.run_case(v) for k, v in sorted(cs.CASES.items())}


@gpu
@pytest.mark.parametrize('case', sorted(cs.CASES))
def test_selection_is_the_parents(ran, case):
    print(case, ran[case]['names'])
    assert ran[case]['names'] == PARENT['cases'][case]['names']


@gpu
@pytest.mark.parametrize('case', sorted(cs.CASES))
def test_outputs_are_bit_identical_to_the_parents(ran, case):
    want = PARENT['cases'][case]
    for what in ('y', 'dx', 'dW'):
        if want[what] is not None:
            assert ran[case][what] == want[what], (case, what)


def test_predicates_answer_as_the_parent():
    if not os.path.exists(nv.LIB_PATH):
        pytest.skip('libsegnb_hip.so not built (run __graft_entry__.build())')
    got = cs.predicate_table()
    assert sorted(got) == sorted(PARENT['predicates'])
    for q in sorted(got):
        a, b = got[q].split(','), PARENT['predicates'][q].split(',')
        assert len(a) == len(b) and len(a) >= 400, q
        diff = [i for i in range(len(a)) if a[i] != b[i]]
        assert not diff, (q, len(diff), diff[:10])


@gpu
def test_refusals_keep_status_message_and_target():
    got = cs.error_paths()
    assert sorted(got) == sorted(PARENT['errors'])
    for name in sorted(got):
        print(name, got[name])
        assert got[name] == PARENT['errors'][name], name
    # the weight-gradient entry points consume the armed target whatever they return; a forward entry point never does
    for name, (rc, msg, delivered) in got.items():
        assert rc == -1 and msg
        assert delivered == (name.startswith('oversize') or name in ('refused_drop', 'refused_upsum')), name
