"""The selection rule of the LDS-DMA forward launchers, csrc/ws_select.h, run without a GPU: a stand-alone host program
(tests/ws_select_host.py) includes the header and prints its choice for a list of launches, and that choice has to equal the rule
of the commit before the header existed (f7c5fec: dispatch_fd, launch_ws, ws_launch_form, ksplit_factor, try_upd,
segnb_fprop_upf_try of csrc/fprop_dma.hip and the ladder of segnb_fprop_rw_try, csrc/fprop_rw.hip) restated here in Python, line
by line, over the geometries of tests/conv_select.py -- the grid of its predicate sweep and its recorded cases -- and over sweeps
of the widths, channel counts, CU counts and knob values at which the rule branches.  default_cfg is that commit's restatement,
checked against its source by the test this file replaced, and stands unchanged.

The 14 x 14-pixel tile (224 matrix rows, cfg 3) may be chosen only inside its gate -- H and W multiples of 14, W <= 56, no
activation mask on the launch -- and, by default, only at the measured levels 14^2, 28^2 and 56^2, where it minimises
rounds x matrix rows per tile, and only for launches whose statistics stay bit for bit: those that take none (data gradients) and
those at 14^2 (one image per tile under both tilings).  None of the geometries recorded before the tile existed lies inside the
gate (the one recorded since that does is named below), so the kernels behind the recorded digests
of tests/conv_select_parent.json are the ones that produced them.  tests/test_ws_tile14_gpu.py and tests/test_conv_select_gpu.py
check on the GPU (call census "tile:...") that the library follows the header at the geometries they run."""
import itertools
import os

import pytest

import conv_select as cs
import ws_select_host as wh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = (256, 128, 25, 5)                    # segnb_knob_conv_cus(): the whole chip, a data-parallel share, 10 % and 2 %
DEFAULT_LEVELS = (14, 28, 56)


def gate(H, W, Co, mask=False):
    """ws14_serves + the default path's own conditions"""
    return H % 14 == 0 and W % 14 == 0 and W <= 56 and Co > 32 and not mask


def default_cfg(N, H, W, Co, cus, mask=False, stats=False):
    """dispatch_fd with fprop_dma_cfg = -1 -> 0 (8 x 32), 1 (16 x 16), 2 (tall 36 x 7), 3 (14 x 14) or None (declined)"""
    if Co <= 32:
        return None
    if W <= 8:
        return 2 if (H, W) == (7, 7) else None
    gm = max(1, cus // ((Co + 63) // 64))
    rounds = lambda tiles: (tiles + gm - 1) // gm
    r0 = rounds(N * ((H + 7) // 8) * ((W + 31) // 32))
    r1 = rounds(N * ((H + 15) // 16) * ((W + 15) // 16))
    cfg = 0 if r0 < r1 else 1
    if mask:
        cfg = 1
    if gate(H, W, Co, mask) and (not stats or W == 14) and H == W and W in DEFAULT_LEVELS:
        r3 = rounds(N * (H // 14) * (W // 14))
        if r3 * 224 < (r0 if cfg == 0 else r1) * 256:
            cfg = 3
    return cfg


def _sweep():
    """(N, H, W, Co) of conv_select.predicate_table's grid: the stride-1 3 x 3 rows, both sides (forward: Co; data gradient: Ci)"""
    for k, stride, dil, *pad in cs.GRID_TAPS:
        if (k, stride) != (3, 1) or pad:          # (the row without padding has outputs of W - 2: only host predicates see it)
            continue
        for W in cs.GRID_W:
            for Ci in cs.GRID_C_IN:
                for Co in cs.GRID_C_OUT:
                    for out_ch in (Co, Ci):
                        yield 2, 8 if W < 16 else W, W, out_ch


@pytest.fixture(scope='module')
def header(tmp_path_factory):
    """ask(queries) -> the answers of ws_select.h's host program"""
    tmp = tmp_path_factory.mktemp('ws_select')
    exe = wh.build(tmp)
    return lambda queries: wh.ask(exe, queries, tmp)


def _timed_step():
    """the levels of the bs = 32 224 x 224 step and the other sizes of test_levels_of_the_timed_step_...: (N, H, W, Co)"""
    for hw, c in ((56, 128), (28, 256), (14, 512)):
        yield 32, hw, hw, c
    for H, W in ((42, 42), (28, 56), (70, 70), (15, 15), (16, 16), (112, 112), (224, 224)):
        yield 32, H, W, 128
    yield 32, 56, 56, 32


def _case_sides():
    for name, case in sorted(cs.CASES.items()):
        dtype, N, H, W, Ci, Co, k, stride = case[:8]
        Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
        yield N, Ho, Wo, Co
        yield N, H, W, Ci


def test_header_is_the_parents_default_rule(header):
    """ws_select at the default knobs == default_cfg over the whole of _sweep() x CUS x mask x statistics, every recorded case
    (both sides) and the levels of the timed step; the constants default_cfg restates (224 rows, the gate, the levels) are thereby
    the header's"""
    geoms = sorted(set(_sweep()) | set(_case_sides()) | set(_timed_step()))
    keys = [(g, cus, mask, stats) for g in geoms for cus in CUS for mask in (False, True) for stats in (False, True)]
    # (a mask comes with its sums: WsFacts::stats is set with it, as segnb_fprop_dma_try does; default_cfg's `stats` is the forward's)
    got = header([wh.ws_query(N, H, W, 64, Co, stats=stats or mask, mask=mask, cus=cus) for (N, H, W, Co), cus, mask, stats in keys])
    assert set(_sweep()) <= set(geoms) and len(keys) == 16 * len(geoms) >= 1200
    for ((N, H, W, Co), cus, mask, stats), c in zip(keys, got):
        want = default_cfg(N, H, W, Co, cus, mask, stats or mask)
        if mask and want is not None and want != 1:
            want = None             # launch_ws (f7c5fec fprop_dma.hip:1417): only the 16 x 16 tile has the MASK instantiation
        assert c.row == want, (N, H, W, Co, cus, mask, stats, c)
        assert c.row != 3 or (c.BM == 224 == (196 + 31) // 32 * 32 and c.tag == 'tile:ws14')


# ---- what default_cfg does not cover: the parent's rule restated from f7c5fec csrc/fprop_dma.hip / fprop_rw.hip -------------------
WIDTHS = (7, 8, 12, 14, 16, 32, 56, 192, 224)
CHANNELS = (32, 64, 96, 256, 1024)


def _flat(N, H, W, cus, ntl):
    """8 x 32 (0) or 16 x 16 (1) by rounds, ties to 16 x 16 (dispatch_fd :1585-1589, try_upd :1541-1545, upf :1658-1662)"""
    gm = max(1, cus // ntl)
    r0 = (N * ((H + 7) // 8) * ((W + 31) // 32) + gm - 1) // gm
    r1 = (N * ((H + 15) // 16) * ((W + 15) // 16) + gm - 1) // gm
    return 0 if r0 < r1 else 1


def parent_row(N, H, W, Ci, Co, cus, cfg=-1, mask=False, stats=False, ep=False, dbg=False, Hi=None, Wi=None):
    """segnb_fprop_dma_try :1730 + dispatch_fd :1560-1619 + launch_ws :1417, :1441 -> 0..3 or None"""
    if Ci % 64:
        return None
    can14 = gate(H, W, Co, mask) and not ep and not dbg                        # ws14_serves :1474-1477
    if cfg == 3 and not can14:
        cfg = -1
    if cfg < 0:
        cfg = default_cfg(N, H, W, Co, cus, mask, stats)
        if cfg == 3 and not can14:
            cfg = 1 if mask else _flat(N, H, W, cus, (Co + 63) // 64)
    if cfg is None or cfg > 3:
        return None
    if mask and cfg != 1:                                                      # MASK_OK :138: 256 rows on four M-waves with 2 KB left
        return None
    if cfg == 2 and (W > 7 or (Hi or H) != H or (Wi or W) != W):               # :1441
        return None
    return cfg


def parent_form(row, stats, mask, ep, dbg, nostats):
    """ws_launch_form :1382-1413 (PAIR for the 14 x 14 row)"""
    if row != 3:
        if mask:
            return wh.MASK
        if ep:
            return wh.EP
    if not stats and not dbg and nostats:
        return wh.NOSTATS
    if row != 3 and dbg:
        return wh.DBG
    return wh.STATS


def parent_epi(row, ep, knob):
    """ws_has_epi :1334-1337 (the 16 x 16 and 14 x 14 rows), ws_epi_selected :1338-1344, launch_ws :1462, launch_ws14 :1488"""
    return row in (1, 3) and not ep and (True if knob < 0 else knob != 0)


def parent_ksplit(N, H, Ci, Co, cus, stats, knob, ep=False, dbg=False):
    """ksplit_factor :1310-1327 on the tall row (IT, NTL of ws_tile_grid :1368)"""
    if not knob or ep or dbg:
        return 1
    tiles = ((N * (H + 1) + 35) // 36) * ((Co + 63) // 64)
    nch = Ci // 64
    if not stats:
        cus //= 2
    ks = 1
    if tiles * 2 <= cus and nch % 2 == 0 and nch // 2 >= 2:
        ks = 2
    if tiles * 4 <= cus and nch % 4 == 0 and nch // 4 >= 2:
        ks = 4
    if knob > 1 and nch % knob == 0 and nch // knob >= 2 and knob in (2, 4):
        ks = knob
    if tiles * ks * 65536 >= 1 << 31:
        return 1
    return ks


def _square(w):
    return (7, 7) if w == 7 else (8, 8) if w == 8 else (w, w)


def test_forced_configurations(header):
    """fprop_dma_cfg 0..3 (and -1, and a value beyond the table): the row, or the decline, is the parent's -- 3 where the 14 x 14
    form does not serve falls back to the default, 0 with a mask declines, 2 beyond 7 columns declines"""
    keys = [(N, w, Co, cus, cfg, mask, stats) for N in (1, 2, 32) for w in WIDTHS for Co in CHANNELS for cus in CUS
            for cfg in (-1, 0, 1, 2, 3, 4) for mask in (False, True) for stats in (False, True)]
    got = header([wh.ws_query(N, *_square(w), 128, Co, stats=stats or mask, mask=mask, cus=cus, cfg=cfg)
                  for N, w, Co, cus, cfg, mask, stats in keys])
    fell_back = declined_mask = 0
    for (N, w, Co, cus, cfg, mask, stats), c in zip(keys, got):
        H, W = _square(w)
        want = parent_row(N, H, W, 128, Co, cus, cfg, mask, stats or mask)
        assert c.row == want, (N, H, W, Co, cus, cfg, mask, stats, c)
        fell_back += cfg == 3 and want is not None and want != 3
        declined_mask += cfg == 0 and mask and want is None
    assert fell_back and declined_mask
    # Ci that is no multiple of 64, and a tall launch whose input is larger than its output (a window without padding)
    assert [c.row for c in header([wh.ws_query(2, 16, 16, 96, 64), wh.ws_query(2, 7, 7, 64, 64, Hi=9, Wi=9),
                                   wh.ws_query(2, 7, 7, 64, 64)])] == [None, None, 2]


def test_forms_and_store_row_order(header):
    """the instantiation form (mask, affine epilogue, none, timing build, statistics) and fprop_dma_epi -1 / 0 / 1 per row"""
    keys = [(w, cfg, stats, mask, ep, dbg, nostats, epi) for w in (7, 14, 16, 32) for cfg in (-1, 0, 1, 2, 3)
            for stats, mask, ep, dbg, nostats in itertools.product((False, True), repeat=5) for epi in (-1, 0, 1)
            if not (mask and ep)]                               # (segnb_fprop_dma_try :1703 declines a mask with an epilogue)
    got = header([wh.ws_query(2, *_square(w), 128, 64, stats=stats or mask, mask=mask, ep=ep, dbg=dbg, cfg=cfg, nostats=nostats, epi=epi)
                  for w, cfg, stats, mask, ep, dbg, nostats, epi in keys])
    seen = set()
    for (w, cfg, stats, mask, ep, dbg, nostats, epi), c in zip(keys, got):
        H, W = _square(w)
        row = parent_row(2, H, W, 128, 64, 256, cfg, mask, stats or mask, ep, dbg)
        assert c.row == row, (w, cfg, stats, mask, ep, dbg, c)
        if row is not None:
            assert c.form == parent_form(row, stats or mask, mask, ep, dbg, nostats), (w, cfg, stats, mask, ep, dbg, nostats, c)
            assert c.epi == parent_epi(row, ep, epi), (w, cfg, ep, epi, c)
            seen.add((row, c.form, c.epi))
    # every instantiation the table lists but split K's (below) is reached: 4 + 9 + 4 + 4
    assert len(seen) == 21, sorted(seen)


def test_split_k_factor(header):
    """all of ksplit_factor's conditions: the knob (0 off, 1 automatic, 2 / 4 forced, 3 ignored), the halved CU budget without
    statistics, chunk counts that the factor does not divide or leaves fewer than two of, the 2 GiB slab bound, no split under the
    affine epilogue or a timing build; and the form it launches (statistics unless fprop_nostats serves a launch without)"""
    keys = [(N, Ci, Co, cus, stats, knob, ep, dbg, nostats) for N in (1, 2, 32, 8192) for Ci in (64, 128, 192, 256, 512, 1024)
            for Co in (64, 256, 1024) for cus in CUS + (64, 16) for stats in (False, True) for knob in (0, 1, 2, 3, 4)
            for ep, dbg in ((False, False), (True, False), (False, True)) for nostats in (0, 1)]
    got = header([wh.ws_query(N, 7, 7, Ci, Co, stats=stats, ep=ep, dbg=dbg, cus=cus, ksplit=knob, nostats=nostats)
                  for N, Ci, Co, cus, stats, knob, ep, dbg, nostats in keys])
    seen = set()
    for (N, Ci, Co, cus, stats, knob, ep, dbg, nostats), c in zip(keys, got):
        assert c.row == 2
        want = parent_ksplit(N, 7, Ci, Co, cus, stats, knob, ep, dbg)
        assert c.ks == want, (N, Ci, Co, cus, stats, knob, ep, dbg, c)
        assert c.ks_form == (wh.KS_STATS if stats or not nostats else wh.KS_NOSTATS)      # launch_ws :1453-1456
        seen.add((want, stats, knob))
    assert {ks for ks, _, _ in seen} == {1, 2, 4}
    # the halved budget: 8 tiles x 4 <= 32 CUs with statistics, not on the 16 that are left without
    assert parent_ksplit(2, 7, 512, 512, 32, True, 1) == 4 and parent_ksplit(2, 7, 512, 512, 32, False, 1) == 2
    # the slab bound: forced slices of a launch whose slabs pass 2 GiB
    assert parent_ksplit(8192, 7, 256, 1024, 256, True, 2) == 1 and parent_ksplit(32, 7, 256, 1024, 256, True, 2) == 2
    # no other row splits
    assert all(c.ks == 1 for c in header([wh.ws_query(1, 16, 16, 512, 64, cfg=cfg) for cfg in (0, 1)] + [wh.ws_query(1, 14, 14, 512, 64)]))


def test_plane_gather_and_phase_forward_tiles(header):
    """try_upd :1533-1548 with upd_geometry :1525-1531 (plane gather: Ci of 64-channel chunks or 32, Co > 32, Wo >= 12) and
    segnb_fprop_upf_try :1631, :1658-1664 (phase forward: four times the channel tiles; Ci >= 128; Co <= 32 only with no_prev)"""
    keys = [(N, w, Ci, Co, cus, cfg, no_prev) for N in (1, 2, 32) for w in WIDTHS for Ci in CHANNELS for Co in CHANNELS
            for cus in CUS for cfg in (-1, 0, 1, 2) for no_prev in (False, True)]
    upd = header([wh.ws_query(N, *_square(w), Ci, Co, Hi=2 * _square(w)[0], Wi=2 * w, window=wh.WIN_UPD, cus=cus, cfg=cfg)
                  for N, w, Ci, Co, cus, cfg, no_prev in keys])
    upf = header([wh.ws_query(N, *_square(w), Ci, Co, stats=True, window=wh.WIN_UPF, no_prev=no_prev, cus=cus, cfg=cfg)
                  for N, w, Ci, Co, cus, cfg, no_prev in keys])
    rows = set()
    for (N, w, Ci, Co, cus, cfg, no_prev), d, f in zip(keys, upd, upf):
        H, W = _square(w)
        want = None
        if (Ci % 64 == 0 or Ci == 32) and Co > 32 and W >= 12:
            want = 4 + (_flat(N, H, W, cus, (Co + 63) // 64) if cfg < 0 else 0 if cfg == 0 else 1)
        assert d.row == want and (want is None or (d.form, d.epi, d.ks) == (wh.NOSTATS, False, 1)), (N, w, Ci, Co, cus, cfg, d)
        want = None
        if Ci % 64 == 0 and Ci >= 128 and (Co > 32 or no_prev) and W >= 12:
            want = 6 + (_flat(N, H, W, cus, 4 * ((Co + 63) // 64)) if cfg < 0 else 0 if cfg == 0 else 1)
        assert f.row == want and (want is None or (f.form, f.epi, f.ks) == (wh.STATS, False, 1)), (N, w, Ci, Co, cus, cfg, no_prev, f)
        rows |= {d.row, f.row}
    assert rows == {None, 4, 5, 6, 7}
    # the gather's other gates: the input is the doubled grid, the taps are in order, no statistics / bias / epilogue come with it
    base = dict(Hi=32, Wi=32, window=wh.WIN_UPD)
    declined = header([wh.ws_query(2, 16, 16, 64, 64, **dict(base, **kw)) for kw in
                       (dict(Hi=16), dict(row_major=False), dict(stats=True), dict(bias=True), dict(ep=True), dict(upd=0), dict(dma=0))])
    assert [c.row for c in declined] == [None] * 7 and header([wh.ws_query(2, 16, 16, 64, 64, **base)])[0].row == 5


def parent_rw(Co, NCH, Wo, stats):
    """segnb_fprop_rw_try :494, :545-562 at rw_store_waves = 4 -> RwCfg<BN, NS, NSW, R, WT> or None"""
    if NCH not in (1, 2, 3) or Co > 96 or Wo < 12:
        return None
    if Co <= 32:
        return (32, 6 - NCH, 4, 8, 32) if Wo >= 192 else (32, 6 - NCH, 4, 16, 16)
    if Co <= 64:
        return (64, 3, 4, 16, 16)
    return None if stats else (96, 2, 2, 16, 16)


def test_rw_rows_are_the_parents_ladder(header):
    keys = [(Co, NCH, Wo, stats) for Co in (8, 16, 32, 40, 64, 72, 96, 104, 256) for NCH in (0, 1, 2, 3, 4) for Wo in WIDTHS + (191,)
            for stats in (False, True)]
    got = header([wh.rw_query(*k) for k in keys])
    tiles = set()
    for k, (row, tile) in zip(keys, got):
        assert (None if row is None else tile) == parent_rw(*k), (k, row, tile)
        tiles.add(row)
    assert tiles == set(range(8)) | {None}


def test_unordered_taps_are_declined(header):
    """the one change of behaviour: a 3 x 3 window whose taps are not row-major was served by the 32x32x16 small-tile forms, which
    are gone; it is declined now whatever else holds"""
    qs = [wh.ws_query(2, w, w, 64, 64, row_major=False, cfg=cfg) for w in (7, 14, 16, 32) for cfg in (-1, 0, 1, 2, 3)]
    assert all(c.row is None for c in header(qs))


def test_host_program_under_sanitizers(tmp_path):
    """the same program built with -fsanitize=address,undefined, run on the CPU as its own process over a sample of every sweep"""
    try:
        exe = wh.build(tmp_path, ('-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g'))
    except Exception as e:      # (a host toolchain without the sanitizer runtimes)
        pytest.skip('no sanitizer runtimes: %s' % e)
    qs = [wh.ws_query(N, *_square(w), Ci, Co, stats=s, mask=m, cus=cus, cfg=cfg, ksplit=ks)
          for N in (1, 8192) for w in WIDTHS for Ci in (64, 1024) for Co in (32, 1024) for s in (False, True) for m in (False, True)
          for cus in (256, 5) for cfg in (-1, 0, 1, 2, 3, 4, 99) for ks in (1, 4)]
    qs += [wh.ws_query(2, 16, 16, 128, 64, Hi=32, Wi=32, window=wh.WIN_UPD), wh.ws_query(2, 16, 16, 128, 64, window=wh.WIN_UPF)]
    qs += [wh.rw_query(Co, NCH, Wo, s) for Co in (32, 64, 96, 128) for NCH in (0, 1, 3, 4) for Wo in (8, 12, 192) for s in (False, True)]
    assert len(wh.ask(exe, qs, tmp_path)) == len(qs)


def test_sweep_never_leaves_the_gate():
    picked = 0
    for N, H, W, Co in _sweep():
        for cus in CUS:
            for mask in (False, True):
                for stats in (False, True):
                    cfg = default_cfg(N, H, W, Co, cus, mask, stats)
                    assert cfg != 3 or gate(H, W, Co, mask), (N, H, W, Co, cus, mask)
                    picked += cfg == 3
    assert picked == 0, 'the sweep\'s widths (8, 12, 16, 32) hold no multiple of 14'


# Recorded on a commit whose dispatch_fd already had the tile, and inside the gate by necessity: the weight gradient's flat
# 14 x 14 configuration exists only at 14 x 14 pixels with more than 32 channels on both sides.  Its digests are the tile's.
RECORDED_WITH_THE_TILE = {'wg_flat14': 3}


def test_recorded_geometries_keep_their_tile():
    assert len(cs.CASES) == 39
    for name, case in cs.CASES.items():
        dtype, N, H, W, Ci, Co, k, stride = case[:8]
        Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
        for n, h, w, co in ((N, Ho, Wo, Co), (N, H, W, Ci)):           # forward, data gradient
            if name in RECORDED_WITH_THE_TILE:
                assert gate(h, w, co) and default_cfg(n, h, w, co, 256) == RECORDED_WITH_THE_TILE[name], name
                continue
            assert not gate(h, w, co), name
            for cus in CUS:
                assert default_cfg(n, h, w, co, cus) != 3 and default_cfg(n, h, w, co, cus, stats=True) != 3, name


def test_levels_of_the_timed_step_take_the_tile_and_nothing_else_does():
    """bs = 32: 56^2 (128 channels), 28^2 (256), 14^2 (512) -> cfg 3 with the tile count of the 16 x 16 form; a mask, another
    size made of 14 x 14 tiles, or a size that is not, stay where they were"""
    for hw, c in ((56, 128), (28, 256), (14, 512)):
        assert default_cfg(32, hw, hw, c, 256) == 3, hw
        assert default_cfg(32, hw, hw, c, 256, stats=True) == (3 if hw == 14 else 1), hw      # forwards: 14^2 only
        for cus in CUS:
            # (a share of the CUs can give the 8 x 32 tiles fewer rounds: 7 x 256 rows against 8 x 224 is a tie, and ties stay)
            assert default_cfg(32, hw, hw, c, cus) in (0, 3), (hw, cus)
            assert default_cfg(32, hw, hw, c, cus, mask=True) == 1
        assert 32 * (hw // 14) ** 2 == 32 * ((hw + 15) // 16) ** 2
    for H, W in ((42, 42), (28, 56), (70, 70), (15, 15), (16, 16), (112, 112), (224, 224)):
        assert default_cfg(32, H, W, 128, 256) in (0, 1), (H, W)
    assert default_cfg(32, 56, 56, 32, 256) is None
