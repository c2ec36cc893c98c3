"""What the convolution entry points of libsegnb_hip.so select, answer and refuse, as data: the cases of
tests/test_conv_select_gpu.py and the functions that run them.

Run as a script on the commit whose behaviour is to be pinned (the PARENT of a change to the host side of csrc/conv_igemm.hip):

    python tests/conv_select.py tests/conv_select_parent.json

It runs everything twice and refuses to write a table the library does not repeat itself.  The weight gradient of a row that the
general kernel serves is left out of the digests (dW: null): that kernel sums with fp32 atomics and is not bit-reproducible.
A table that exists is widened, not replaced: the script refuses to write unless it reproduces every row the table already holds.
"""
import hashlib
import json
import os
import sys

if __name__ == '__main__':
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(_ROOT, 'segmentation-networks-benchmark_amd'), _ROOT]

import torch

from segnb import _native as nv
from segnb import convplan as cp

JSON_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'conv_select_parent.json')
DW_EXCLUDED = 'kernel:wgrad_general sums with fp32 atomics: the parent does not repeat its own bits'

# ------------------------------------------------------------------------------------------------ 1 + 3. selection and bits
# id: (dtype, N, H, W, Ci, Co, kernel, stride, bias and statistics in the forward[, segnb_tune knobs set around the launches])
CASES = {
    'dma_64_64': ('bf16', 2, 16, 16, 64, 64, 3, 1, True),
    'rw_32_64': ('bf16', 2, 12, 20, 32, 64, 3, 1, True),
    'deepk_256_256': ('bf16', 1, 8, 8, 256, 256, 3, 1, True),
    'c8_8_32': ('bf16', 2, 16, 16, 8, 32, 3, 1, True),
    'c8roll_8_32': ('bf16', 2, 16, 32, 8, 32, 3, 1, True),
    'general_16_64_plain': ('bf16', 2, 16, 16, 16, 64, 3, 1, False),
    'roll_32_32': ('bf16', 2, 16, 32, 32, 32, 3, 1, True),
    'wroll_32_32': ('bf16', 2, 16, 32, 32, 32, 3, 1, True, {'wgrad_roll': 1}),      # (the knob is off by default: runtime.hip)
    's1_128_32': ('bf16', 2, 16, 16, 128, 32, 3, 1, True),
    's1_128_32_plain': ('bf16', 2, 16, 16, 128, 32, 3, 1, False),
    's1_48_48': ('bf16', 2, 16, 16, 48, 48, 3, 1, True),
    'general_stride2': ('bf16', 2, 16, 16, 64, 64, 3, 2, True),
    'wsx_1x1': ('bf16', 2, 16, 16, 64, 64, 1, 1, True),
    'general_f32': ('f32', 2, 12, 20, 32, 64, 3, 1, True),
    # fprop_thin.hip thin_geometry: a data gradient of 16 -> >= 48 channels over N * Ho * Wo >= 4096 pixels, no bias or statistics
    'thin_48_16': ('bf16', 2, 32, 64, 48, 16, 3, 1, True),
    # fprop_sx.hip segnb_fprop_sx_try: in_step == 2, 8 input channels, QW >= 24 (an input 48 wide)
    'sx_8_32_stride2': ('bf16', 1, 8, 48, 8, 32, 3, 2, True),
    # wgrad_s1.hip s1_choose: one geometry per row of its configuration table
    'wg_thin_r8': ('bf16', 2, 24, 32, 64, 32, 3, 1, True),           # Co <= 32, Wo >= 24, Ho % 16 != 0
    'wg_thin_r16': ('bf16', 1, 64, 32, 64, 32, 3, 1, True),          # Ho % 16 == 0 and Ho >= 64
    'wg_wide_r4': ('bf16', 2, 20, 40, 64, 64, 3, 1, True),           # Ho divisible by neither 8 nor 7
    'wg_wide_r8_ragged': ('bf16', 2, 16, 40, 72, 40, 3, 1, True),    # Ho % 8 == 0; ragged channels in both tiles
    'wg_wide_r7': ('bf16', 2, 14, 40, 64, 64, 3, 1, True),           # Ho % 7 == 0, Wo > 16
    'wg_w16_wide': ('bf16', 2, 16, 48, 64, 64, 3, 1, True),          # Wo % 16 == 0, Wo % 32 != 0
    'wg_w16_narrow': ('bf16', 2, 12, 12, 64, 64, 3, 1, True),        # 12 <= Wo <= 16, not 14 x 14
    'wg_flat14': ('bf16', 2, 14, 14, 64, 64, 3, 1, True),
    'wg_flat7': ('bf16', 5, 7, 7, 64, 64, 3, 1, True),               # four images per iteration: the last one is ragged
    # wgrad_s1.hip sx_choose: the rows this format can express (the 4 x 4 stride-2 and 2 x 2 rows: test_strided_wgrad_takes_the_tile_kernel)
    'wsx_1x1_16': ('bf16', 2, 16, 16, 16, 64, 1, 1, True),
    'wsx_1x1_32': ('bf16', 2, 16, 16, 32, 64, 1, 1, True),
    'wsx_1x1_128': ('bf16', 2, 16, 16, 128, 64, 1, 1, True),         # ('wsx_1x1' above is the 64-channel row)
    'wsx_3x3s2_w32': ('bf16', 2, 48, 48, 32, 64, 3, 2, True),        # Wo = 24
    'wsx_3x3s2_w16': ('bf16', 2, 24, 24, 32, 64, 3, 2, True),        # Wo = 12
    'wsx_7x7s2': ('bf16', 2, 64, 64, 8, 64, 7, 2, True),             # the stem, Wo >= 32
    # fprop_dma.hip WS_ROWS (ws_select.h: ws_select): the rows this format can express ('dma_64_64': 16 x 16, 'wg_flat14': 14 x 14)
    'ws_8x32': ('bf16', 2, 24, 32, 64, 64, 3, 1, True, {'conv_cu_pct': 1}),      # two persistent blocks: 3 rounds of 8 x 32 against 4
    'ws_tall_ksplit': ('bf16', 2, 7, 7, 256, 64, 3, 1, True),        # 7 x 7 images: the tall row, four chunks in two slices
    # fprop_rw.hip RW_ROWS (ws_select.h: rw_select): one geometry per row ('rw_32_64': <64,3,4>)
    'rw_32_32': ('bf16', 2, 12, 20, 32, 32, 3, 1, True),             # <32,5,4>
    'rw_64_32': ('bf16', 2, 12, 20, 64, 32, 3, 1, True),             # <32,4,4>
    'rw_96_32': ('bf16', 2, 12, 20, 96, 32, 3, 1, True),             # <32,3,4>; its data gradient (32 -> 96): <96,2>
    # (Wo >= 192.  The rolling-window kernel stands in front of this one in the cascade and takes 32 and 64 input channels at this
    # size -- recorded as such: <32,5,4,8,32> and <32,4,4,8,32> are rows this format does not reach at the default knobs)
    'rw_wide_32_32': ('bf16', 1, 8, 192, 32, 32, 3, 1, True),
    'rw_wide_64_32': ('bf16', 1, 8, 192, 64, 32, 3, 1, True),
    'rw_wide_96_32': ('bf16', 1, 8, 192, 96, 32, 3, 1, True),        # <32,3,4,8,32>
}
# what segnb_tune keys of a case go back to after its launches
KNOB_DEFAULTS = {'wgrad_roll': 0, 'conv_cu_pct': 100}
# selectors that no case above reaches, and the gate that keeps them away
UNREACHED = {}
# rows of fprop_dma.hip's table that the case format cannot express: the gate, and the test that runs them
WS_ROWS_UNREACHED = {
    'tile:ws_upd8x32': 'plane gather (ntaps 16, in_step 2: segnb.engine.UpConvOp data gradient): fused_table() "act upconv T4x4 s2 relu", '
                       'test_hip_ops.py',
    'tile:ws_upd16': 'plane gather, the 16 x 16 tile: test_hip_ops.py',
    'tile:ws_upf8x32': 'phase forward (segnb_upconv_fprop): fused_table() "act upconv T4x4 s2 relu", test_hip_ops.py',
    'tile:ws_upf16': 'phase forward, the 16 x 16 tile: test_hip_ops.py',
}
# forms of the rows above that the case format cannot express
WS_FORMS_UNREACHED = {
    'mask': 'activation mask (segnb_conv_fprop_bnreduce without coefficients): test_ws_epi_gpu.py, test_ws_tile_switch_gpu.py',
    'affine epilogue': 'segnb_conv_fprop_act: fused_table() "act ..." rows, test_hip_ops.py',
    'virtual concat': 'segnb_conv_fprop_upcat: fused_table() "upcat ..." rows',
}
FPROP_SELECTORS = ['kernel:fprop_' + s for s in ('c8', 'thin', 'roll', 'rw', 'dma', 'deepk', 's1', 'sx', 'general')]
WGRAD_SELECTORS = ['kernel:wgrad_' + s for s in ('roll', 'c8roll', 's1', 'sx', 'general')]


def _randn(shape, seed, scale=1.0):
    """bf16-exact fp32 values from a fixed-seed CPU generator"""
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).bfloat16().float()


def _sha(t):
    t = t.detach().contiguous().cpu()
    t = t.view(torch.int16) if t.dtype == torch.bfloat16 else t
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


class census(object):
    def __enter__(self):
        nv.call('segnb_tune', b'call_census', 1)
        nv.census_read()
        return self

    def take(self):
        """the selectors counted since the last take; self.tiles: the table rows of fprop_dma.hip counted beside them"""
        c = nv.census_read()
        self.tiles = {k: v for k, v in c.items() if k.startswith('tile:')}
        return {k: v for k, v in c.items() if k.startswith('kernel:')}

    def __exit__(self, *a):
        nv.call('segnb_tune', b'call_census', 0)


def _operands(rt, case, seed=0):
    """(op, x view with ld != C, dy view, H, W of the output) of a case, weights packed"""
    from segnb.engine import ConvOp, View
    dtype, N, H, W, Ci, Co, k, stride, full = case[:9]
    dev = rt.device
    w = _randn((Co, Ci, k, k), 71 + seed, (2.0 / (Ci * k * k)) ** 0.5).to(dev)
    b = _randn((Co,), 72 + seed).to(dev) if full else None
    op = ConvOp(rt, w, b, [(Ci, Ci)], stride, (k - 1) // 2, False, need_dgrad=True)
    op.pack(H, W)
    Ho, Wo = op.out_hw(H, W)
    ld = Ci + 8
    xv = View(rt.zeros((N, H, W, ld)), N, H, W, Ci, ld, 8)
    xv.dense().copy_(_randn((N, H, W, Ci), 73 + seed).to(dev, rt.tdtype))
    dyv = View.alloc(rt, N, Ho, Wo, Co)
    dyv.dense().copy_(_randn((N, Ho, Wo, Co), 74 + seed).to(dev, rt.tdtype))
    return op, xv, dyv, Ho, Wo


def run_case(case, tiles=None):
    """-> {'names': [forward, data gradient, weight gradient census], 'y', 'dx', 'dW': SHA-256 of the output bytes}; tiles (a list)
    receives the "tile:..." census of the forward and of the data gradient"""
    from segnb.engine import Runtime, View
    dtype, N, H, W, Ci, Co, k, stride, full = case[:9]
    knobs = case[9] if len(case) > 9 else {}
    rt = Runtime(torch.device('cuda:0'), dtype)
    op, xv, dyv, Ho, Wo = _operands(rt, case)
    yv, dxv = View.alloc(rt, N, Ho, Wo, Co), View.alloc(rt, N, H, W, Ci)
    stats = rt.zeros((16, 2, Co), torch.float64) if full else None
    gw = torch.zeros_like(op.weight)
    for knob, v in knobs.items():
        nv.call('segnb_tune', knob.encode(), v)
    try:
        with census() as c:
            op.fprop(xv, yv, stats)
            kf = c.take()
            tf = c.tiles
            op.dgrad(dyv, dxv)
            kd = c.take()
            if tiles is not None:
                tiles += [tf, c.tiles]
            op.wgrad(xv, dyv, gw)
            kw = c.take()
    finally:
        for knob in knobs:
            nv.call('segnb_tune', knob.encode(), KNOB_DEFAULTS[knob])
    torch.cuda.synchronize()
    out = {'names': [kf, kd, kw], 'y': _sha(yv.dense()), 'dx': _sha(dxv.dense()), 'dW': _sha(gw)}
    if 'kernel:wgrad_general' in kw:
        out['dW'], out['dW_excluded'] = None, DW_EXCLUDED
    return out


# ------------------------------------------------------------------------------------------------ 2. predicates
GEOM_QUERIES = ('segnb_conv_fprop_drop_ok', 'segnb_conv_fprop_bnreduce_ok', 'segnb_conv_fprop_bnapply_ok',
                'segnb_conv_fprop_actmask_ok', 'segnb_conv_fprop_u8_ok', 'segnb_conv_fprop_upd_ok', 'segnb_conv_wgrad_bnapply_ok',
                'segnb_conv_wgrad_tf_ok', 'segnb_conv_wgrad_slabs')
CU_QUERIES = ('segnb_conv_upcat_ok', 'segnb_conv_fprop_upsum_ok')                 # (g, dtype, Cu)
UPCONV_QUERIES = ('segnb_upconv_fprop_ok', 'segnb_upconv_fprop_acc_ok')           # (N, H, W, Ci, Co, ld_out, dtype)
TF_QUERY = 'segnb_conv_fprop_tf_ok'                                               # (g, dtype, kind)
GRID_C_IN, GRID_C_OUT, GRID_W = (8, 16, 32, 64, 96, 128, 512), (8, 32, 64, 96, 256), (8, 12, 16, 32)
# (kernel, stride, dilation[, pad]); pad = dilation * ((kernel - 1) // 2) unless given.  The last row is a window without padding
# (linknet.py:60): its forward origin is 0 and its data-gradient origin -2, beside the -1 of the padded rows
GRID_TAPS = ((3, 1, 1), (3, 2, 1), (1, 1, 1), (3, 1, 2), (4, 2, 1), (3, 1, 1, 0))
GRID_CU = (8, 32, 64)


def _geom(N, H, W, Ci, Co, k, stride, dil, side='f', pad=None):
    from segnb.engine import ConvOp
    pad = dil * ((k - 1) // 2) if pad is None else pad
    (Ho, Wo), fwd = cp.conv_fwd(H, W, k, k, stride, pad, dil)
    if side == 'f':
        return ConvOp._make_geom(fwd[0], N, H, W, Ci, Ci, Ho, Wo, Co, Co)
    return ConvOp._make_geom(cp.conv_dgrad(H, W, k, k, stride, pad, dil)[0][0], N, Ho, Wo, Co, Co, H, W, Ci, Ci)


def predicate_table():
    """{query: its answers over the grid in grid order, comma-separated}; nothing is launched"""
    lib = nv.load()
    out = {q: [] for q in GEOM_QUERIES + CU_QUERIES + UPCONV_QUERIES + (TF_QUERY,)}
    for k, stride, dil, *pad in GRID_TAPS:
        for W in GRID_W:
            for Ci in GRID_C_IN:
                for Co in GRID_C_OUT:
                    for side in 'fd':
                        g = _geom(2, 8 if W < 16 else W, W, Ci, Co, k, stride, dil, side, *pad)
                        for dt in (nv.BF16, nv.F32):
                            for q in GEOM_QUERIES:
                                out[q].append(getattr(lib, q)(g, dt))
                        for q in CU_QUERIES:
                            out[q] += [getattr(lib, q)(g, nv.BF16, cu) for cu in GRID_CU]
                        out[TF_QUERY] += [getattr(lib, TF_QUERY)(g, nv.BF16, kind) for kind in (nv.TF_ACT, nv.TF_BNBWD)]
    for W in GRID_W:
        for Ci in GRID_C_IN:
            for Co in GRID_C_OUT:
                for q in UPCONV_QUERIES:
                    out[q] += [getattr(lib, q)(2, W, W, Ci, Co, Co + pad, nv.BF16) for pad in (0, 8)]
                    out[q].append(getattr(lib, q)(2, W, W, Ci, Co, Co, nv.F32))
    return {q: ','.join(str(v) for v in a) for q, a in out.items()}


# ------------------------------------------------------------------------------------------------ 4. error paths
def error_paths():
    """{name: [status, message, did a following un-armed segnb_conv_wgrad deliver into the parameter's gradient]}: every call below
    is refused before it launches anything; a segnb_wgrad_target is armed in front of each"""
    from segnb.engine import Runtime, View
    lib = nv.load()
    rt = Runtime(torch.device('cuda:0'), 'bf16')
    case = CASES['dma_64_64']
    dtype, N, H, W, Ci, Co = case[:6]
    op, xv, dyv, Ho, Wo = _operands(rt, case)
    p = op.plan(H, W)
    g = op._launch_geom(p, 'f', 0, N, H, W, xv.ld, dyv.ld)
    yv = View.alloc(rt, N, Ho, Wo, Co)
    dwp, nslab, wp, st = nv.ptr(p['dwp'][0]), p['nslab'][0], nv.ptr(p['wp_fwd'][0]), rt.stream
    assert op.direct_ok()

    huge = _geom(1, 16384, 16384, 8, 8, 3, 1, 1)                  # 2^28 pixels x 8 channels x 2 bytes = 4 GiB
    wide = _geom(N, H, W, Ci, Co, 3, 1, 1)                        # 64 output channels: what segnb_conv_fprop_drop_ok refuses
    src = nv.UpcatSrc(xv.ptr, Ci, Ci)                             # Cu == Ci: what segnb_conv_upcat_ok refuses
    calls = {
        'oversize_plain': lambda: lib.segnb_conv_fprop(huge, nv.BF16, xv.ptr, wp, None, 0, yv.ptr, None, st),
        'oversize_upconv': lambda: lib.segnb_upconv_fprop(nv.BF16, 1, 64, 64, 128, 1 << 19, xv.ptr, wp, 64, 64, None, 0, yv.ptr, 64,
                                                          None, st),
        'refused_drop': lambda: lib.segnb_conv_fprop_drop(wide, nv.BF16, xv.ptr, wp, None, 0, yv.ptr, xv.ptr, Co, None, 0, st),
        'refused_upsum': lambda: lib.segnb_conv_fprop_upsum(wide, nv.BF16, xv.ptr, wp, yv.ptr, src, st),
        'refused_wgrad_upcat': lambda: lib.segnb_conv_wgrad_upcat(g, nv.BF16, xv.ptr, src, dyv.ptr, dwp, nslab, st),
        'refused_wgrad_tf': lambda: lib.segnb_conv_wgrad_tf(g, nv.BF16, xv.ptr, None, dyv.ptr, None, dwp, nslab, st),
        'nslab_differs': lambda: lib.segnb_conv_wgrad(g, nv.BF16, xv.ptr, dyv.ptr, dwp, nslab + 1, st),
    }
    out = {}
    for name in sorted(calls):
        gw = torch.zeros_like(op.weight)
        p['dwp'][0].zero_()
        op._arm_target(p, 0, gw)
        rc = calls[name]()
        msg = (lib.segnb_last_error() or b'').decode()
        nv.call('segnb_conv_wgrad', g, nv.BF16, xv.ptr, dyv.ptr, dwp, nslab, st)
        torch.cuda.synchronize()
        delivered, in_workspace = bool(gw.abs().sum() > 0), bool(p['dwp'][0][0].abs().sum() > 0)
        assert delivered or in_workspace, name
        out[name] = [rc, msg, delivered]
    return out


# ------------------------------------------------------------------------------------------------ 5. the fused entry points
# Tensors of a row that are sum tables written with fp64 atomics, by the name the driver gives them.  One that the parent does not
# repeat is left out of the digests (null, and named in the row's 'excluded'); any other tensor has to repeat.
FUSED_SUM_TABLES = ('stats', 'sums', 'stats virtual', 'stats segment')
FUSED_EXCLUDED = 'a sum table written with fp64 atomics: the parent does not repeat its own bits'
FUSED_ACT_CASES = ('rw 32->64 relu', 'upconv T4x4 s2 relu')       # test_hip_ops.ACT_EP_CASES: a plain and a ConvTranspose2d(4, 2, 1) case


def _digests(d):
    return {k: _sha(v) for k, v in sorted(d.items()) if torch.is_tensor(v)}


def _conv_op_launches():
    """one segnb_conv_fprop_drop, one segnb_conv_fprop_u8 (with the packed pixels) and one segnb_conv_fprop_bnreduce launch through
    ConvOp, each at a small shape its *_ok accepts -> {row: {tensor: torch tensor}}"""
    from segnb.engine import ConvOp, InputNorm, Runtime, View
    rt = Runtime(torch.device('cuda:0'), 'bf16')
    dev, out = rt.device, {}

    def conv(Co, Ci, segs, bias, seed, dgrad):
        w = _randn((Co, Ci, 3, 3), seed, (2.0 / (Ci * 9)) ** 0.5).to(dev)
        return ConvOp(rt, w, _randn((Co,), seed + 1).to(dev) if bias else None, segs, 1, 1, False, need_dgrad=dgrad)

    def filled(N, H, W, C, seed):
        v = View.alloc(rt, N, H, W, C)
        v.dense().copy_(_randn((N, H, W, C), seed).to(dev, rt.tdtype))
        return v

    # conv -> Dropout2d -> slice statistics: <= 32 output channels behind more than 96 input channels (segnb_conv_fprop_drop_ok)
    N, H, W, C1, C2 = 2, 16, 16, 128, 16
    op = conv(C2, C1, [(C1, C1)], True, 81, False)
    op.pack(H, W)
    LD, OFF = C1 + C2 + 24, C1
    cat, table = View.alloc(rt, N, H, W, LD), rt.zeros((16, 2, LD), torch.float64)
    drop = (_randn((N, C2), 83) > -0.8).float().mul(1.25).to(dev)
    assert op.drop_epilogue_ok(N, H, W, LD)
    op.fprop_drop(filled(N, H, W, C1, 84), cat.slice(OFF, C2), drop, (table, OFF, LD))
    out['fprop_drop 2x16x16 128->16'] = {'y': cat.t, 'stats': table.sum(0)}
    # the first layer from the uint8 batch (segnb_conv_fprop_u8_ok: 8 padded channels -> <= 32, at least 12 wide)
    N, H, W = 2, 16, 16
    img = torch.randint(0, 256, (N, H, W, 3), generator=torch.Generator().manual_seed(85), dtype=torch.uint8).to(dev)
    op = conv(32, 3, [(3, 8)], True, 86, False)
    op.pack(H, W)
    assert op.u8_direct_ok(N, H, W, 32)
    xp, yv, st = View.alloc(rt, N, H, W, 8), View.alloc(rt, N, H, W, 32), rt.zeros((16, 2, 32), torch.float64)
    op.fprop_u8(img, InputNorm(), yv, st, xp)
    out['fprop_u8 2x16x16 3->32'] = {'y': yv.t, 'packed': xp.t, 'stats': st.sum(0)}
    # a data gradient with the BatchNorm-backward reduction of the producing layer in its store pass (segnb_conv_fprop_bnreduce_ok)
    N, H, W, C = 2, 16, 32, 32
    op = conv(C, C, [(C, C)], False, 88, True)
    op.pack(H, W)
    dyv, dxv, y1 = filled(N, H, W, C, 90), View.alloc(rt, N, H, W, C), filled(N, H, W, C, 91)
    coef = torch.stack([0.5 + _randn((C,), 92).abs(), _randn((C,), 93, 0.3), _randn((C,), 94, 0.2), 0.5 + _randn((C,), 95).abs()])
    coef, sums = coef.contiguous().to(dev), rt.zeros((16, 2, C), torch.float64)
    assert op.dgrad_bnreduce_ok(dyv, dxv)
    op.dgrad(dyv, dxv, bn_reduce=(y1, coef, sums, nv.ACT_LEAKY, 0.01))
    out['dgrad bn_reduce 2x16x32 32->32'] = {'dx': dxv.t, 'sums': sums.sum(0)}
    torch.cuda.synchronize()
    return out


def fused_table():
    """{row: {tensor: SHA-256 of its bytes}}: every stored tensor the drivers of tests/fused_errbound.py produce at their smallest
    served shapes, and the three launches of _conv_op_launches"""
    import fused_errbound as fe
    from test_hip_ops import ACT_EP_CASES
    out = {}
    s = fe.THIN_SERVED[0]
    dx, dx_f, sums = fe.run_thin('cuda', s, fe.thin_data(s))
    out['thin ' + fe.sid(s)] = _digests({'dx': dx, 'dx fused': dx_f, 'sums': sums})
    s = fe.TF_SHAPES[1]
    for use_drop in (False, True):
        out['tf %s%s' % (fe.sid(s), ' drop' if use_drop else '')] = _digests(fe.run_tf('cuda', s, fe.tf_data(s, use_drop)))
    for s in (fe.UPCAT_SHAPES[0], fe.UPCAT_SHAPES[2]):
        out['upcat ' + fe.sid(s)] = _digests(fe.run_upcat('cuda', s, fe.upcat_data(s)))
    acts = {c[0]: c for c in ACT_EP_CASES}
    for name in FUSED_ACT_CASES:
        for with_bn in (False, True):
            y, buf, coef = fe.run_act('cuda', acts[name], 'bf16', with_bn, fe.act_data(acts[name], 'bf16'))
            # (the one-launch transposed convolution takes no folded BatchNorm: run_act asserts that its gate says so)
            out['act %s%s' % (name, ' evalbn' if with_bn else '')] = {'served': False} if y is None else _digests({'y': y, 'buffer': buf})
    for row, tensors in _conv_op_launches().items():
        out[row] = _digests(tensors)
    return out


def fused_without_unrepeated_sums(*runs):
    """the first of several fused_table() results with the sum tables that differ between them left out; anything else that
    differs is an error"""
    out = {}
    for row, first in runs[0].items():
        out[row] = dict(first)
        for k in first:
            if any(r[row][k] != first[k] for r in runs[1:]):
                assert k in FUSED_SUM_TABLES, ('not reproducible', row, k)
                out[row][k] = None
                out[row]['excluded'] = FUSED_EXCLUDED
    return out


def record():
    return {'cases': {k: run_case(v) for k, v in sorted(CASES.items())}, 'predicates': predicate_table(), 'errors': error_paths(),
            'fused': fused_table()}


if __name__ == '__main__':
    a, b = record(), record()
    for k in a['cases']:
        print(k, a['cases'][k]['names'])
        assert a['cases'][k] == b['cases'][k], ('not reproducible', k, a['cases'][k], b['cases'][k])
    assert a['predicates'] == b['predicates'] and a['errors'] == b['errors']
    for k, v in sorted(a['errors'].items()):
        print(k, v)
    a['fused'] = fused_without_unrepeated_sums(a['fused'], b['fused'], fused_table())
    for k, v in sorted(a['fused'].items()):
        print(k, sorted(t for t in v if v[t] is None), len(v))
    seen = {n for c in a['cases'].values() for side in c['names'] for n in side}
    print('selectors not reached:', sorted(set(FPROP_SELECTORS + WGRAD_SELECTORS) - seen))
    assert seen | set(UNREACHED) == set(FPROP_SELECTORS + WGRAD_SELECTORS), sorted(set(FPROP_SELECTORS + WGRAD_SELECTORS) - seen)
    if os.path.exists(JSON_PATH):
        # a table that is being widened: what it already holds is reproduced as it stands (a predicate's answers over a longer
        # grid begin with the answers it had)
        with open(JSON_PATH) as f:
            old = json.load(f)
        for k, v in old['cases'].items():
            assert a['cases'][k] == v, ('the table\'s row is not reproduced', k, a['cases'][k], v)
        assert all(a['errors'][k] == v for k, v in old['errors'].items())
        assert all((a['predicates'][q] + ',').startswith(v + ',') for q, v in old['predicates'].items())
        assert all(a['fused'][k] == v for k, v in old.get('fused', {}).items())
    with open(sys.argv[1] if len(sys.argv) > 1 else JSON_PATH, 'w') as f:
        json.dump(a, f, indent=0, sort_keys=True, separators=(',', ':'))
        f.write('\n')
