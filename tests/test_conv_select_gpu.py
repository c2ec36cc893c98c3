"""The host side of the convolution entry points (csrc/conv_igemm.hip) against a table recorded on the commit before its helpers
were factored out (tests/conv_select_parent.json, written by tests/conv_select.py on that commit; never by the code under test):

  1. which kernel serves the forward, data gradient and weight gradient of small geometries that between them reach every
     selector of the two plain cascades (those that no small geometry reaches: conv_select.UNREACHED, with the gate);
  2. the answer of every fast-path query over a grid of geometries -- host functions, so this one runs without a GPU too;
  3. SHA-256 of the output bytes of every launch of 1: the kernels and their arguments did not change, so neither do the bits
     (left out: weight gradients of the general kernel, which sums with fp32 atomics -- named in the table);
  4. status and message of the refusals that moved into helpers, and which call consumes an armed segnb_wgrad_target;
  6. which row of fprop_dma.hip's table served a recorded case is the row csrc/ws_select.h names for that geometry at the device's
     CU count (tests/test_ws_tile14_cpu.py: the header is the parent's rule; here: the library follows the header; 3: the bits are
     the parent's); and a 3 x 3 window whose taps are not in row-major order is declined by fprop_dma.hip and served within bounds.
  5. SHA-256 of every stored tensor of the fused entry points at their smallest served shapes (conv_select.fused_table: the drivers
     of tests/fused_errbound.py and three ConvOp launches); a sum table the parent does not repeat is named in its row.
"""
import json
import os

import pytest
import torch

import conv_select as cs
import errbound as eb
import ws_select_host as wh
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
    """every case once: {id: run_case(), with the "tile:..." census of its forward and data gradient under 'tiles'}"""
    out = {}
    for k, v in sorted(cs.CASES.items()):
        tiles = []
        out[k] = dict(cs.run_case(v, tiles), tiles=tiles)
    return out


@pytest.fixture(scope='module')
def header_rows(tmp_path_factory):
    """{id: [Choice of the forward, Choice of the data gradient]} of csrc/ws_select.h for the stride-1 3 x 3 bf16 cases, at the CUs
    segnb_knob_conv_cus() gives the case (runtime.hip: segnb_device_cus() * conv_cu_pct / 100)"""
    tmp = tmp_path_factory.mktemp('ws_select')
    names = [k for k, c in sorted(cs.CASES.items()) if c[0] == 'bf16' and c[6:8] == (3, 1)]
    cus_all = nv.load().segnb_device_cus()
    queries = []
    for k in names:
        dtype, N, H, W, Ci, Co, _, _, full = cs.CASES[k][:9]
        cus = cus_all * (cs.CASES[k][9] if len(cs.CASES[k]) > 9 else {}).get('conv_cu_pct', 100) // 100
        queries += [wh.ws_query(N, H, W, Ci, Co, stats=full, bias=full, cus=cus), wh.ws_query(N, H, W, Co, Ci, cus=cus)]
    got = wh.ask(wh.build(tmp), queries, tmp)
    return {k: got[2 * i:2 * i + 2] for i, k in enumerate(names)}


@gpu
@pytest.mark.parametrize('case', sorted(cs.CASES))
def test_table_row_is_the_one_the_header_names(ran, header_rows, case):
    names, tiles = ran[case]['names'], ran[case]['tiles']
    print(case, names[:2], tiles, header_rows.get(case))
    for side in (0, 1):
        if 'kernel:fprop_dma' not in names[side]:
            assert tiles[side] == {}, (case, side)
            continue
        want = header_rows[case][side]
        assert want.row is not None and tiles[side] == {want.tag: 1}, (case, side, want)


def test_recorded_cases_reach_the_rows_the_format_can_express():
    """fprop_dma.hip's rows by what ws_select.h names for the recorded geometries on a whole MI355X; the others are listed with
    their gate and the tests that run them"""
    assert set(cs.WS_ROWS_UNREACHED) == {'tile:ws_upd8x32', 'tile:ws_upd16', 'tile:ws_upf8x32', 'tile:ws_upf16'}
    assert all(cs.WS_ROWS_UNREACHED.values()) and all(cs.WS_FORMS_UNREACHED.values())
    for name, side in (('ws_8x32', 0), ('dma_64_64', 0), ('ws_tall_ksplit', 0), ('wg_flat14', 1)):        # 8 x 32, 16 x 16, tall, 14 x 14
        assert PARENT['cases'][name]['names'][side] == {'kernel:fprop_dma': 1}, name


@gpu
def test_unordered_taps_are_declined_and_served_within_bounds():
    """64 -> 64 at 2 x 16 x 16 with the nine taps in column-major order and the packed weights permuted to match: fprop_dma.hip
    declines (the 32x32x16 small-tile forms that took such a list are gone), the next kernel of the cascade takes
    the taps as they are, and the output lies within the derived bound of tests/errbound.py against F.conv2d"""
    from segnb.engine import ConvOp, Runtime, View
    N, H, W, C = 2, 16, 16, 64
    rt = Runtime(torch.device('cuda:0'), 'bf16')
    w, b = cs._randn((C, C, 3, 3), 171, (2.0 / (C * 9)) ** 0.5), cs._randn((C,), 172)
    x = cs._randn((N, C, H, W), 173)
    op = ConvOp(rt, w.to(rt.device), b.to(rt.device), [(C, C)], 1, 1, False, need_dgrad=False)
    p = op.plan(H, W)
    launch = p['fwd'][0]
    order = [3 * (t % 3) + t // 3 for t in range(9)]
    p['fwd'][0] = launch._replace(taps=[launch.taps[t] for t in order])
    assert [tap[:2] for tap in p['fwd'][0].taps[:3]] == [(-1, -1), (0, -1), (1, -1)]           # (dh, dw): down the first column
    p['tapoff_fwd'][0] = nv.int_array(op._taps(p['fwd'][0]))
    op.pack(H, W)
    xv, yv = View.alloc(rt, N, H, W, C), View.alloc(rt, N, H, W, C)
    xv.dense().copy_(x.permute(0, 2, 3, 1).to(rt.device, rt.tdtype))
    with cs.census() as c:
        op.fprop(xv, yv, None)
        served = c.take()
        torch.cuda.synchronize()
    print(served, c.tiles)
    assert 'kernel:fprop_dma' not in served and c.tiles == {} and len(served) == 1, served
    ref = eb.conv_refs(x, w, b, torch.zeros(N, C, H, W), 1, 1, False)
    got = yv.dense().float().cpu().permute(0, 3, 1, 2)
    worst = eb.assert_within_bound('column-major taps', got, ref['y'], ref['mag_y'], ref['K_y'], 'bf16')
    print('worst err / bound %.3f' % worst)


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
