"""-m gpu: the convolutions that have an element-wise pass fused into them against float64 references under DERIVED per-element
bounds, and exactly on probe operands (tests/fused_errbound.py holds the derivations and the constructions;
tests/test_conv_fused_errbound_cpu.py proves them on the CPU and shows that the emulator wrong in one place fails them).

  thin data gradient      conv_thin_kernel (fprop_thin.hip) plain and with the BatchNorm-reduce epilogue: dx under errbound's
                          bound, equal bits from both launches, the sums against float64 sums of dz from the STORED dx
  consumer-side BatchNorm segnb_conv_fprop_tf (SEGNB_TF_ACT forward, SEGNB_TF_BNBWD data gradient) and segnb_conv_wgrad_tf
                          against a float64 operand oracle; the bound is widened only by the convolution of the operand's slack
  virtual concat          segnb_conv_fprop_upcat / _wgrad_upcat, segnb_upconv_fprop_acc, the segmented data gradient (skip and
                          low-resolution du) and segnb_conv_fprop_upsum against conv2d(cat(interpolate(u), skip)) with the
                          weights the kernels multiply by (phase matrices rounded after their fp32 sum)
  activation epilogues    segnb_conv_fprop_act / segnb_upconv_fprop_act with and without folded eval-mode BatchNorm

The shapes are the small rows of test_hip_ops.py; conv_thin_kernel serves 4096 pixels and more (thin_geometry), which none of
those reaches, so two shapes just past that gate are added and the kernel that served each launch is read from the census."""
import os

import pytest

import fused_errbound as fe
from conv_select import census
from test_hip_ops import ACT_EP_CASES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIO_FILE = os.path.join(ROOT, 'profiles', 'fused_errbound_ratios.txt')
RATIOS = {}          # (family, dtype, tensor) -> (worst err / bound, case name)
FORMS = {}           # form of the decoder's first convolution -> the shapes it served
BOUND_RUNS = set()   # ids of the bound tests that ran to their end

THIN_RUNS = fe.THIN_SHAPES + fe.THIN_SERVED
TF_RUNS = [(s, dr) for s in fe.TF_SHAPES for dr in (False, True)]
ACT_RUNS = [(c, bn, dt) for c in ACT_EP_CASES for bn in (False, True) for dt in ('f32', 'bf16') if dt == 'bf16' or 'upconv' not in c[0]]
N_BOUND_RUNS = len(THIN_RUNS) + len(TF_RUNS) + len(fe.UPCAT_SHAPES) + len(ACT_RUNS)


@pytest.fixture(scope='session', autouse=True)
def recorded_ratios():
    """the worst err / bound per family, dtype and tensor of this session -> profiles/fused_errbound_ratios.txt when
    SEGNB_RECORD_ERRBOUND=1 (measurements: the threshold is 1 and is derived)"""
    yield
    # the record is a tracked file: rewritten only on request, and only by a complete run of the module
    if os.environ.get('SEGNB_RECORD_ERRBOUND') != '1' or len(BOUND_RUNS) < N_BOUND_RUNS:
        return
    lines = ['# worst err/bound of tests/test_conv_fused_errbound_gpu.py per family, dtype and tensor (bounds: tests/fused_errbound.py;',
             '# sums: |sums - float64 sum over the stored tensor| / (P * 2^-23 * magnitude)).  Measurements, not thresholds: the',
             '# threshold is 1.  "thin dgrad" rows are launches that kernel:fprop_thin served, "dense-layer dgrad (general)" the',
             '# same layer at fewer than 4096 pixels.',
             '# Written by: SEGNB_RECORD_ERRBOUND=1 pytest -m gpu tests/test_conv_fused_errbound_gpu.py',
             '# family | dtype | tensor | worst ratio | case']
    for (fam, dtype, tensor), (r, name) in sorted(RATIOS.items()):
        lines.append('%-28s | %-4s | %-12s | %.4f | %s' % (fam, dtype, tensor, r, name))
    lines.append('# forms of the decoder\'s first convolution and the shapes that reached them')
    for form in fe.UPCAT_FORMS:
        lines.append('# %-20s %s' % (form, ' '.join(FORMS.get(form, []))))
    with open(RATIO_FILE, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def _done(run_id, name, res, rename=None):
    ratios, msgs = res
    for (fam, dtype, tensor), r in ratios.items():
        key = ((rename or {}).get(fam, fam), dtype, tensor)
        if key not in RATIOS or r > RATIOS[key][0]:
            RATIOS[key] = (r, name)
        print('%s | %s | %s | %s: err/bound %.4f' % (key + (name, r)))
    BOUND_RUNS.add(run_id)
    assert not msgs, '\n'.join(msgs)


@pytest.mark.parametrize('shape', THIN_RUNS, ids=fe.sid)
def test_thin_dgrad_within_derived_bound(shape):
    with census() as c:
        res = fe.check_thin('cuda', shape, census=c)
    served = 'kernel:fprop_thin' in c.seen and 'kernel:fprop_thin' in c.seen_fused
    print('%s: plain launch %s, fused launch %s' % (fe.sid(shape), sorted(c.seen), sorted(c.seen_fused)))
    if shape in fe.THIN_SERVED:
        assert served, 'conv_thin_kernel does not serve %s: %s / %s' % (fe.sid(shape), sorted(c.seen), sorted(c.seen_fused))
    _done('thin ' + fe.sid(shape), fe.sid(shape), res, None if served else {'thin dgrad': 'dense-layer dgrad (general)'})


@pytest.mark.parametrize('shape', THIN_RUNS, ids=fe.sid)
def test_thin_dgrad_impulses_exact(shape):
    _, msgs = fe.check_thin_impulses('cuda', shape)
    assert not msgs, '\n'.join(msgs)


@pytest.mark.parametrize('shape,use_drop', TF_RUNS, ids=['%s|%s' % (fe.sid(s), 'drop' if dr else 'nodrop') for s, dr in TF_RUNS])
def test_tf_within_widened_bound(shape, use_drop):
    _done('tf %s %s' % (fe.sid(shape), use_drop), fe.sid(shape) + (' drop' if use_drop else ''), fe.check_tf('cuda', shape, use_drop))


@pytest.mark.parametrize('shape,use_drop', TF_RUNS, ids=['%s|%s' % (fe.sid(s), 'drop' if dr else 'nodrop') for s, dr in TF_RUNS])
def test_tf_impulses_exact(shape, use_drop):
    _, msgs = fe.check_tf_impulses('cuda', shape, use_drop)
    assert not msgs, '\n'.join(msgs)


@pytest.mark.parametrize('shape,use_drop', TF_RUNS, ids=['%s|%s' % (fe.sid(s), 'drop' if dr else 'nodrop') for s, dr in TF_RUNS])
def test_tf_wgrad_probe_exact(shape, use_drop):
    _, msgs = fe.check_tf_wgrad_probe('cuda', shape, use_drop)
    assert not msgs, '\n'.join(msgs)


def test_every_upcat_form_is_served_by_a_shape():
    """the gates of UpCatConvOp (virtual, fwd_segmented, segmented, upsum) on this device: nothing is launched"""
    for shape in fe.UPCAT_SHAPES:
        for form, ok in fe.upcat_forms('cuda', shape).items():
            if ok:
                FORMS.setdefault(form, []).append(fe.sid(shape))
    print(FORMS)
    assert set(FORMS) == set(fe.UPCAT_FORMS), 'not served at any shape: %s' % sorted(set(fe.UPCAT_FORMS) - set(FORMS))


@pytest.mark.parametrize('shape', fe.UPCAT_SHAPES, ids=fe.sid)
def test_upcat_within_derived_bound(shape):
    _done('upcat ' + fe.sid(shape), fe.sid(shape), fe.check_upcat('cuda', shape))


@pytest.mark.parametrize('shape', fe.UPCAT_SHAPES, ids=fe.sid)
def test_upcat_impulses_exact(shape):
    _, msgs = fe.check_upcat_impulses('cuda', shape)
    assert not msgs, '\n'.join(msgs)


@pytest.mark.parametrize('case,with_bn,dtype', ACT_RUNS, ids=['%s|%s|%s' % (c[0], 'evalbn' if bn else 'act', dt) for c, bn, dt in ACT_RUNS])
def test_act_epilogue_within_derived_bound(case, with_bn, dtype):
    _done('act %s %s %s' % (case[0], with_bn, dtype), case[0], fe.check_act('cuda', case, dtype, with_bn))
