"""The default tile selection of dispatch_fd (csrc/fprop_dma.hip) restated in Python and evaluated without a GPU over the
geometries of tests/conv_select.py: the grid of its predicate sweep and its recorded cases.

The 14 x 14-pixel tile (224 matrix rows, cfg 3) may be chosen only inside its gate -- H and W multiples of 14, W <= 56, no
activation mask on the launch -- and, by default, only at the measured levels 14^2, 28^2 and 56^2, where it minimises
rounds x matrix rows per tile, and only for launches whose statistics stay bit for bit: those that take none (data gradients) and
those at 14^2 (one image per tile under both tilings).  None of the geometries recorded before the tile existed lies inside the
gate (the one recorded since that does is named below), so the kernels behind the recorded digests
of tests/conv_select_parent.json are the ones that produced them.  tests/test_ws_tile14_gpu.py checks on the GPU (call census
"tile:ws14") that the library follows the same rule at the geometries it runs."""
import os
import re

import conv_select as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'segmentation-networks-benchmark_amd', 'csrc', 'fprop_dma.hip')
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


def test_rule_matches_the_source():
    """the constants restated above are the ones in dispatch_fd / ws14_serves / WsCfg14"""
    src = open(SRC).read()
    assert 'using WsCfg14 = WsCfg<64, 14, 14, 2, false, true>;' in src
    assert re.search(r'a\.H % 14 == 0 && a\.W % 14 == 0 && a\.W <= 56 && a\.Co > 32 && a\.bn_y == nullptr', src)
    assert 'constexpr unsigned WS14_DEFAULT_LEVELS = 7u;' in src          # bits 0..2: 14, 28, 56
    assert 'if (r3 * WsCfg14::BM < (cfg == 0 ? r0 : r1) * 256) cfg = 3;' in src
    assert 'const bool same_stats = a.stats == nullptr || a.W == 14;' in src
    assert (196 + 31) // 32 * 32 == 224                                    # WsCfg::BM of 14 x 14 pixels on two M-waves


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
    assert len(cs.CASES) == 31
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
