"""The host side of the element-wise entry points (csrc/norm_act.hip, csrc/elementwise.hip, csrc/head_loss.hip and the three
packers with a dtype argument) against a table recorded on the commit before their dtype dispatch, parameter blocks and launch
geometry were each said once (tests/ew_table_parent.json, written by tests/ew_table.py on that commit; never by the code under
test):

  A. SHA-256 of every output buffer of every row -- one row per branch of a host-side dispatch, on the BN_CASES shapes of
     tests/test_hip_ops.py, in bf16 and fp32; the table keeps, per row and dtype, one SHA-256 over those of its outputs.
     The kernels and their arguments did not change, so neither do the bits.  Every tensor is a view into a wider
     sentinel-filled buffer and the digest covers the buffer.
  B. status and message of the refusals, character for character; host code, so this part runs wherever the library loads.
"""
import json
import os
import re

import pytest

import ew_table as ew
from segnb import _native as nv

with open(ew.JSON_PATH) as f:
    PARENT = json.load(f)

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the entry points that moved to csrc/elementwise.hip without a family prefix of their own
MOVED = ['segnb_add', 'segnb_nhwc_to_nchw_f32', 'segnb_sgd_step', 'segnb_rmsprop_step', 'segnb_adam_step']
FAMILIES = r'segnb_(bn|head|abn|maxpool|upsample)_\w+'
QUERIES = {'segnb_head_fused_ok', 'segnb_head_conv_ok'}             # answers, not launches: no output to digest


def _declared():
    """the entry points of the families as include/segnb_hip.h declares them"""
    with open(os.path.join(ROOT, 'include', 'segnb_hip.h')) as f:
        names = set(re.findall(r'\bint\s+(%s)\s*\(' % FAMILIES, f.read()))
    return {m[0] for m in names}


def test_table_has_a_row_for_every_case_and_every_entry_point():
    assert sorted(PARENT['rows']) == sorted(ew.ROWS)
    called = {e for r in PARENT['rows'].values() for e in r['entries']}
    declared = (_declared() | set(MOVED)) - QUERIES - {'segnb_bias_grad_job_bytes'}
    assert len(declared) >= 38 and {'segnb_bn_act_fwd', 'segnb_head_conv_bwd', 'segnb_maxpool_bwd_add'} <= declared      # (the header was read)
    unreached_entries = {k for k in ew.UNREACHED if k.startswith('segnb_')}
    assert declared <= called | unreached_entries, sorted(declared - called - unreached_entries)
    # both dtypes of every row that takes one
    for row, r in PARENT['rows'].items():
        assert sorted(r['sha']) == sorted(ew.row_dtypes(row)) and all(len(h) == 64 for h in r['sha'].values()), row
    assert sum(len(r['sha']) for r in PARENT['rows'].values()) == len(ew.CASES)


def test_exclusions_are_per_channel_tables_and_few():
    total = left_out = 0
    for row, r in PARENT['rows'].items():
        assert r['outputs'], row
        total += len(r['outputs']) + len(r['excluded'])
        left_out += len(r['excluded'])
        for name, why in r['excluded'].items():
            assert name in ew.EXCLUDABLE and name not in ew.PIXEL_OUTPUTS and why, (row, name)
        assert not set(r['excluded']) & set(r['outputs']), row
    assert left_out * 10 <= total, (left_out, total)
    assert {k for (_, k) in ew.EXCLUDED} <= set(ew.EXCLUDABLE)


def test_unreached_branches_name_their_gate():
    assert 'maxpool_bwd_idx_kernel<T, false>' in ew.UNREACHED
    assert all(gate for gate in ew.UNREACHED.values())


@pytest.fixture(scope='module')
def ran():
    """every case once: {id: run_case()}"""
    return {c: ew.run_case(c) for c in ew.CASES}


@gpu
@pytest.mark.parametrize('row', sorted(ew.ROWS))
def test_outputs_are_bit_identical_to_the_parents(ran, row):
    want, got = PARENT['rows'][row], ew.table_row(row, ran)
    for dt in ew.row_dtypes(row):
        print(row, dt, ran['%s:%s' % (row, dt)]['sha'])             # (the per-output digests, should the row's differ)
    assert got['entries'] == want['entries'] and got['outputs'] == want['outputs'] and got['excluded'] == want['excluded'], row
    for dt in ew.row_dtypes(row):
        assert got['sha'][dt] == want['sha'][dt], (row, dt)


def _same_refusals(got, want):
    assert sorted(got) == sorted(want)
    for name in sorted(got):
        print(name, got[name])
        assert got[name] == want[name], name
        assert got[name][1] == -1 and got[name][2], name            # SEGNB_E_BADARG and a message


def test_refusals_keep_status_and_message():
    if not os.path.exists(nv.LIB_PATH):
        pytest.skip('libsegnb_hip.so not built (run __graft_entry__.build())')
    _same_refusals(ew.refusals(), PARENT['refusals'])
    kinds = {name.split('/')[0] for name in PARENT['refusals']}
    assert {'dtype', 'cp', 'null', 'no_gradient_source', 'residual_and_pooled', 'fused_head', 'stats_ld', 'own_buffer',
            'maxpool_bwd_add', 'head', 'head_conv'} <= kinds
    # an unknown dtype at every dtype-taking entry point of the table
    takes_dtype = {e for row, r in PARENT['rows'].items() if not row.startswith(ew.F32_ONLY) for e in r['entries']}
    refused = {v[0] for k, v in list(PARENT['refusals'].items()) + list(PARENT['gpu_refusals'].items()) if k.startswith('dtype/')}
    assert takes_dtype <= refused, sorted(takes_dtype - refused)


@gpu
def test_refusals_behind_a_device_call_keep_status_and_message():
    _same_refusals(ew.gpu_refusals(), PARENT['gpu_refusals'])
