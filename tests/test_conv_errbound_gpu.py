"""-m gpu: the convolution kernels against float64 references under a DERIVED per-element bound, and exactly on impulse operands
(tests/errbound.py holds the derivation and the constructions; tests/test_errbound_cpu.py proves both on the CPU).

check() of test_hip_ops.py allows 2e-2 of the tensor's maximum on every bf16 element: 10 to 35 times the rounding error the
arithmetic can produce, wide enough for a kernel that drops one product per output.  Here every element of y and dx is held to
    r_out * |ref| * (1 + 2^-8) + K * 2^-23 * sum |a_i b_i| * (1 + r_out) + 2^-126
which any fp32 summation order of the K exact products satisfies, and operands that leave ONE product per output element are
compared with `==`: the only check that sees a lost product behind thousands of terms (the deep-K shapes).

The shapes are the case tables of test_hip_ops.py (each the smallest that reaches its kernel), with the kernel families forced
the way the tests there force them.  The head kernels and the element-wise passes round more than once: they are held to a
float64 oracle in tests/test_ew_oracle_gpu.py (exact operands, `==`) and tests/test_ew_errbound_gpu.py (dense operands, derived
bound).  The convolutions with an element-wise pass fused into them -- the thin data gradient and its BatchNorm-reduce epilogue,
the operands recomputed on load (tf), the virtual concat and the segmented / upsum forms of the decoder's first convolution, the
activation epilogues -- are held to derived bounds and exact probes of their own in tests/test_conv_fused_errbound_gpu.py
(tests/fused_errbound.py).  Four variants stay covered by bit-equality to a composition whose parts are under an oracle, in
test_hip_ops.py: the drop epilogue, the activation mask, wgrad_bnapply and the never-stored data gradient (bnsums / bnapply)."""
import os

import pytest
import torch

import errbound as eb
from segnb import _native as nv
from segnb.engine import ConvOp, Runtime, View
from test_hip_ops import ACT_EP_CASES, CONV_CASES, DEEPK_CASES, DMA_CASES, DTYPES, RW_CASES, _run_conv, check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIO_FILE = os.path.join(ROOT, 'profiles', 'errbound_ratios.txt')
RATIOS = {}          # (family, dtype, tensor) -> (worst err / bound, case name)
BOUND_RUNS = set()   # ids of the entries test_conv_within_derived_bound has measured

KNOB_DEFAULTS = {'fprop_dma': 1, 'fprop_dma_cfg': -1, 'fprop_rw': 1, 'fprop_ksplit': 1, 'fprop_deepk': 1}


@pytest.fixture(scope='session', autouse=True)
def recorded_ratios():
    """the worst err / bound per kernel family and dtype of this session -> profiles/errbound_ratios.txt when SEGNB_RECORD_ERRBOUND=1
    (measurements: the threshold is 1 and is derived)"""
    yield
    # the record is a tracked file: rewritten only on request, and only by a complete run of the module
    if os.environ.get('SEGNB_RECORD_ERRBOUND') != '1' or len(BOUND_RUNS) < len(PROBES):
        return
    lines = ['# worst err/bound of tests/test_conv_errbound_gpu.py per family, dtype and tensor (bound: tests/errbound.py;',
             '# sums: |stats - float64 sum of the stored y| / (P * 2^-23 * sum |y|)).  Measurements, not thresholds: the threshold is 1.',
             '# A family is a group of cases of the tables, named for the bf16 kernel the group was written to reach, or a forced',
             '# knob setting -- not the kernel that was observed to serve the launch.  f32 rows exist only for groups whose kernel',
             '# has an f32 form; the f32 runs of the bf16-only groups are counted under "general".',
             '# Written by: SEGNB_RECORD_ERRBOUND=1 pytest -m gpu tests/test_conv_errbound_gpu.py',
             '# family | dtype | tensor | worst ratio | case']
    for (fam, dtype, tensor), (r, name) in sorted(RATIOS.items()):
        lines.append('%-28s | %-4s | %-6s | %.4f | %s' % (fam, dtype, tensor, r, name))
    with open(RATIO_FILE, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def _record(fam, dtype, tensor, ratio, name):
    key = (fam, dtype, tensor)
    if key not in RATIOS or ratio > RATIOS[key][0]:
        RATIOS[key] = (ratio, name)


class knobs(object):
    """segnb_tune settings for the duration of a block; the knobs the block set are back at their defaults afterwards"""

    def __init__(self, kv):
        self.kv = kv

    def __enter__(self):
        try:
            for k, v in self.kv.items():
                nv.call('segnb_tune', k.encode(), v)
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *a):
        for k in self.kv:
            nv.call('segnb_tune', k.encode(), KNOB_DEFAULTS[k])


BF16_ONLY = ('c8 roll (wgrad_roll)', 'roll', 'deep K shape, with sums', 'upconv', 'c8')       # groups whose kernel has no f32 form


def _family(name):
    for key, fam in (('c8 roll', 'c8 roll (wgrad_roll)'), ('roll', 'roll'), ('deep K', 'deep K shape, with sums'), ('upf', 'upconv'),
                     ('convT', 'convT phases'), ('s1x9', 's1x9'), ('1x1 tile', '1x1 tile'), (' tile', 'strided tile'),
                     ('stem', 'stem'), ('co1', 'co<=8'), ('co6', 'co<=8'), ('co8', 'co<=8'), ('first layer', 'c8')):
        if key in name:
            return fam
    return 'general'


def _7x7(name, N, Ci, Co):
    return (name, N, 7, 7, [(Ci, Ci)], Co, 3, 1, 1, False)


# (family, knobs, case, dtype, forward only without statistics)
TABLE = [('general' if d == 'f32' and _family(c[0]) in BF16_ONLY else _family(c[0]), {}, c, d, False)
         for c in CONV_CASES for d in DTYPES]
FORCED = [('dma cfg %d' % cfg, {'fprop_dma': 1, 'fprop_dma_cfg': cfg}, eb.full_case(c), 'bf16', False)
          for c in DMA_CASES for cfg in (-1, 0, 1)]
FORCED += [('rw', {'fprop_rw': 1}, eb.full_case(c), 'bf16', False) for c in RW_CASES]
FORCED += [('upconv', {}, c, 'bf16', False) for c in ACT_EP_CASES if 'upconv' in c[0]]
FORCED += [('dma tall 7x7', {}, _7x7('tall 7x7 a', 5, 128, 72), 'bf16', False),
           ('dma tall 7x7', {}, _7x7('tall 7x7 b', 9, 64, 200), 'bf16', False)]
# fprop_ksplit: 0 = never split, 1 = the library's own choice, n = n slices where n divides the shape's channel chunks and leaves
# two per slice, else the library's own choice again -- at (5, 256, 72), four chunks, that makes 4 the same launch as 1 and 2;
# at (9, 512, 200) the library's own choice is 4
KSPLIT = {0: 'split K off', 1: 'split K auto', 2: 'split K 2 (where it applies)', 4: 'split K 4 (where it applies)'}
FORCED += [(KSPLIT[ks], {'fprop_ksplit': ks}, _7x7('split K 7x7 %dx%dx%d' % shape, *shape), 'bf16', False)
           for shape in ((5, 256, 72), (9, 512, 200)) for ks in (0, 1, 2, 4)]
FORCED += [('deepk kernel', {'fprop_deepk': 1}, c, 'bf16', True) for c in DEEPK_CASES]
PROBES = TABLE + FORCED
WG_PROBES = TABLE + [e for e in FORCED if e[0] in ('dma cfg -1', 'rw', 'dma tall 7x7')]


def _id(e):
    return '%s|%s|%s' % (e[0], e[2][0], e[3])


def _forward_only(dtype, case, w, b, x):
    """the forward without statistics into a channel slice of a wider buffer (what conv_fprop_deepk_kernel serves) -> y, the
    buffer around it"""
    name, N, H, W, segs, Co, k, s, p, transposed = case
    rt = Runtime('cuda', dtype)
    op = ConvOp(rt, w.cuda(), b.cuda(), segs, s, p, transposed, need_dgrad=False)
    op.pack(H, W)
    Ho, Wo = op.out_hw(H, W)
    xv = View(rt.zeros((N, H, W, op.Cip + 8)), N, H, W, op.Cip, op.Cip + 8, 8)
    off, roff = 0, 0
    for real, padded in segs:
        xv.dense()[..., off:off + real] = x[:, roff:roff + real].permute(0, 2, 3, 1).to('cuda', rt.tdtype)
        off += padded
        roff += real
    ybuf = rt.zeros((N, Ho, Wo, op.Cop + 16))
    yv = View(ybuf, N, Ho, Wo, op.Cop, op.Cop + 16, 8)
    op.fprop(xv, yv, None)
    torch.cuda.synchronize()
    return yv.dense().float().cpu(), ybuf.float().cpu()


def _run(entry, w, b, x, dy):
    """-> y [N,Ho,Wo,Cop], sums [2,Cop] or None, dx [N,H,W,Cip] or None, dW or None"""
    fam, kv, case, dtype, fwd_only = entry
    with knobs(kv):
        if fwd_only:
            y, buf = _forward_only(dtype, case, w, b, x)
            assert float(buf[..., :8].abs().max()) == 0.0 and float(buf[..., 8 + y.shape[-1]:].abs().max()) == 0.0
            return y, None, None, None
        y, st, dx, gw, _, _ = _run_conv('cuda', dtype, case, w, b, x, dy)
    return y, st, dx, gw


def _pad_zero(msgs, what, t, C):
    if t.shape[-1] > C and float(t[..., C:].abs().max()) != 0.0:
        msgs.append('%s: pad channels not zero (max %g)' % (what, float(t[..., C:].abs().max())))


@pytest.mark.parametrize('entry', PROBES, ids=_id)
def test_conv_within_derived_bound(entry):
    """y and dx element by element under the derived bound against float64; pad channels exactly zero; dW against the float64
    weight gradient under the f32 tolerance of check() (fp32 on both dtypes' paths); the epilogue's BatchNorm sums against
    float64 sums of the stored y under the longest fp32 chain a tile could have."""
    fam, kv, case, dtype, fwd_only = entry
    name, N, H, W, segs, Co, k, s, p, transposed = case
    w, b, x, dy = eb.operands(case, dtype)
    r = eb.conv_refs(x, w, b, dy, s, p, transposed)
    y, st, dx, gw = _run(entry, w, b, x, dy)
    msgs = []
    ratio, m = eb.within_bound(name + ' y', y[..., :Co].permute(0, 3, 1, 2), r['y'], r['mag_y'], r['K_y'], dtype)
    _record(fam, dtype, 'y', ratio, name)
    msgs.append(m)
    _pad_zero(msgs, name + ' y', y, Co)
    if dx is not None:
        dxr, pads = eb.real_channels(dx, segs)
        ratio, m = eb.within_bound(name + ' dx', dxr, r['dx'], r['mag_dx'], r['K_dx'], dtype)
        _record(fam, dtype, 'dx', ratio, name)
        msgs.append(m)
        if pads != 0.0:
            msgs.append('%s dx: pad channels not zero (max %g)' % (name, pads))
    if st is not None:
        P = y.shape[0] * y.shape[1] * y.shape[2]
        v = y.double().reshape(P, -1)
        for row, tensor, tot, mag in ((0, 'sum', v.sum(0), v.abs().sum(0)), (1, 'sumsq', (v * v).sum(0), (v * v).sum(0))):
            lim = P * eb.U_ACC * mag + eb.TINY
            rat = (st[row].double() - tot).abs() / lim
            _record(fam, dtype, tensor, float(rat.max()), name)
            if not bool((rat <= 1.0).all()):
                bad = ~(rat <= 1.0)
                msgs.append('%s %s of the epilogue: %d/%d channels over P * 2^-23 * magnitude, worst ratio %.3g, first %s' % (
                    name, tensor, int(bad.sum()), bad.numel(), float(rat.max()), bad.nonzero()[:4].flatten().tolist()))
    BOUND_RUNS.add(_id(entry))
    msgs = [m for m in msgs if m]
    if gw is not None:
        try:
            check(name + ' dW vs float64', gw, r['dW'], 'f32')
        except AssertionError as e:
            msgs.append(str(e))
    assert not msgs, '\n'.join(msgs)


@pytest.mark.parametrize('entry', PROBES, ids=_id)
def test_conv_impulses_exact_fprop_dgrad(entry):
    """x (and dy) zero but for impulses 2^j at least k apart, in another channel at every position, until every real channel
    has carried one: every output is one exact product, so y == round_out(fp32(w * 2^j) + b) and dx == round_out(w * 2^j) in
    any summation order -- compared with ==."""
    fam, kv, case, dtype, fwd_only = entry
    name, N, H, W, segs, Co, k, s, p, transposed = case
    Ci = sum(q for q, _ in segs)
    Ho, Wo = eb.out_size(case)
    w, b, x_dense, _ = eb.operands(case, dtype)
    npass = eb.impulse_passes(N, Ci, H, W, k)
    if not fwd_only:
        npass = max(npass, eb.impulse_passes(N, Co, Ho, Wo, k))
    msgs = []
    for pas in range(npass):
        x = eb.impulse_tensor(N, Ci, H, W, k, pas)
        dy = eb.impulse_tensor(N, Co, Ho, Wo, k, pas)
        y, _, dx, _ = _run(entry, w, b, x, dy)
        msgs.append(eb.mismatches('%s y pass %d' % (name, pas), y[..., :Co].permute(0, 3, 1, 2),
                                  eb.impulse_expect_y(x, w, b, s, p, transposed, dtype)))
        _pad_zero(msgs, name + ' y', y, Co)
        if dx is not None:
            dxr, pads = eb.real_channels(dx, segs)
            msgs.append(eb.mismatches('%s dx pass %d' % (name, pas), dxr, eb.impulse_expect_dx(x, w, dy, s, p, transposed, dtype)))
            if pads != 0.0:
                msgs.append('%s dx: pad channels not zero (max %g)' % (name, pads))
        if len([m for m in msgs if m]) >= 4:
            break
    msgs = [m for m in msgs if m]
    assert not msgs, '\n'.join(msgs)


@pytest.mark.parametrize('entry', WG_PROBES, ids=_id)
def test_conv_impulses_exact_wgrad(entry):
    """x with exactly one non-zero pixel 2^j per input channel, over as many launches as it takes -- 8 at three channels -- to
    place the corners of the first and last image, the ragged last row segment and both sides of the strip, row and pixel-tile
    seams (errbound.essential_pixels; the coverage is asserted in test_errbound_cpu.py), dy dense: every dW[co,ci,ky,kx] is one product or zero, hence equal to the float64 weight gradient
    through slabs, atomics and unpack alike."""
    fam, kv, case, dtype, fwd_only = entry
    name, N, H, W, segs, Co, k, s, p, transposed = case
    Ci = sum(q for q, _ in segs)
    w, b, _, dy = eb.operands(case, dtype)
    msgs = []
    for pas in range(eb.wgrad_probe_passes(N, Ci, H, W)):
        x = eb.wgrad_probe_tensor(N, Ci, H, W, pas)
        _, _, _, gw = _run(entry, w, b, x, dy)
        msgs.append(eb.mismatches('%s dW pass %d' % (name, pas), gw, eb.wgrad_expect(x, w, dy, s, p, transposed)))
    msgs = [m for m in msgs if m]
    assert not msgs, '\n'.join(msgs)
