"""ConvOp's description of its two packed matrices (segnb.engine: ConvOp._form / _taps / _job), checked on CPU against a
recording stand-in for the library: the eager calls (pack(), the unpack of wgrad()) and the batched job records
(pack_jobs(), unpack_jobs()) must describe the same matrices, launch by launch; UpConvOp differs by its masked tap words
only; UpCatConvOp picks its segments' jobs by form."""
import pytest
import torch

from segnb import _native as nv
import segnb.engine as E


class Recorder(object):
    """ABI stand-in: every call is recorded and succeeds, a query answers from `answers` (default 0; one weight-gradient slab)"""

    def __init__(self, **answers):
        self.calls, self.answers = [], dict(segnb_conv_wgrad_slabs=1, **answers)

    def __getattr__(self, name):
        if name in nv.PLAIN:
            return lambda *a: self.answers.get(name, 0)
        return lambda *a: self.calls.append((name, a)) and 0

    def named(self, name):
        return [a for n, a in self.calls if n == name]


@pytest.fixture
def lib(monkeypatch):
    monkeypatch.setattr(E.ConvOp, 'direct_dw', False)
    monkeypatch.setattr(E.UpCatConvOp, 'force_segmented', False)
    rec = Recorder()
    nv.set_backend_for_testing(rec)
    yield rec
    nv.set_backend_for_testing(None)


def _ops(rt):
    """name -> (op, input H, W)"""
    g = torch.Generator().manual_seed(0)
    w = lambda *s: torch.randn(*s, generator=g)
    return {
        'plain3x3': (E.ConvOp(rt, w(5, 3, 3, 3), w(5), [(3, 8)]), 6, 7),                          # Ci = 3 padded to 8, Co = 5
        'stride2': (E.ConvOp(rt, w(6, 4, 3, 3), None, [(4, 8)], stride=2), 7, 6),
        'convt421': (E.ConvOp(rt, w(4, 6, 4, 4), None, [(4, 8)], stride=2, pad=1, transposed=True), 8, 8),
    }


def _same(job, w, packed, Mp, Cp, ntaps, s_m, s_c, tap, mmap, cmap):
    assert (Mp, Cp, ntaps, s_m, s_c) == (job['Mp'], job['Cp'], job['ntaps'], job['s_m'], job['s_c'])
    assert list(tap) == list(job['tap_off']) and len(tap) == ntaps
    assert (w, packed, mmap, cmap) == tuple(job[k].data_ptr() for k in ('w', 'packed', 'mmap', 'cmap'))


@pytest.mark.parametrize('name', ['plain3x3', 'stride2', 'convt421'])
def test_pack_calls_equal_pack_jobs(lib, name):
    op, H, W = _ops(E.Runtime('cpu', 'bf16'))[name]
    op.pack(H, W)
    calls, jobs = lib.named('segnb_pack_weight'), op.pack_jobs(H, W)
    p = op.plan(H, W)
    assert len(calls) == len(jobs) == len(p['fwd']) + len(p['dg'])
    assert [j['form'] for j in jobs] == ['f'] * len(p['fwd']) + ['d'] * len(p['dg'])
    for (w, packed, dtype, Mp, Cp, ntaps, s_m, s_c, tap, mmap, cmap, _), job in zip(calls, jobs):
        _same(job, w, packed, Mp, Cp, ntaps, s_m, s_c, tap, mmap, cmap)
        assert dtype == job['dtype'] == nv.BF16 and 'masked' not in job and 'nslab' not in job
    # the matrices are the plan's, forward then data gradient, and each is [padded rows][taps x padded columns]
    assert [j['packed'].data_ptr() for j in jobs] == [t.data_ptr() for t in p['wp_fwd'] + p['wp_dg']]
    assert all(tuple(j['packed'].shape) == (j['Mp'], j['ntaps'] * j['Cp']) for j in jobs)


@pytest.mark.parametrize('name', ['plain3x3', 'stride2', 'convt421'])
def test_unpack_calls_equal_unpack_jobs(lib, name):
    rt = E.Runtime('cpu', 'bf16')
    op, H, W = _ops(rt)[name]
    Ho, Wo = op.out_hw(H, W)
    gw = torch.zeros(op.weight.shape)
    op.wgrad(E.View.alloc(rt, 2, H, W, op.Cip), E.View.alloc(rt, 2, Ho, Wo, op.Cop), gw, unpack=True)
    calls, jobs = lib.named('segnb_unpack_wgrad'), op.unpack_jobs(H, W, gw)
    p = op.plan(H, W)
    launches = p['dg'] if op.transposed else p['fwd']
    assert len(calls) == len(jobs) == len(launches) == len(lib.named('segnb_conv_wgrad'))
    for (packed, w, Mp, Cp, ntaps, s_m, s_c, tap, mmap, cmap, nslab, _), job in zip(calls, jobs):
        _same(job, w, packed, Mp, Cp, ntaps, s_m, s_c, tap, mmap, cmap)
        assert nslab == job['nslab'] == 1 and job['dtype'] == nv.F32 and 'form' not in job and 'masked' not in job
    assert [j['packed'].data_ptr() for j in jobs] == [t.data_ptr() for t in p['dwp']]
    assert all(j['mmap'] is (op.in_map if op.transposed else op.out_map) for j in jobs)


def test_upconv_jobs_are_masked_and_in_the_data_gradient_form(lib):
    rt = E.Runtime('cpu', 'bf16')
    weight = torch.randn(5, 7, 3, 3)                   # the 3x3 parameter of the whole concat; the op covers 3 of its 7 inputs
    op = E.UpConvOp(rt, weight, 3, 8)
    p = op.plan(4, 4)
    words = lambda ls: [[E.UpConvOp.mask(a, b) for (_, _, a, b) in l.taps] for l in ls]
    jobs = op.pack_jobs(4, 4)
    assert len(jobs) == len(p['fwd']) + len(p['dg']) and all(j['masked'] is True for j in jobs)
    assert [j['tap_off'] for j in jobs] == words(p['fwd']) + words(p['dg'])
    assert [j['form'] for j in jobs] == ['f'] * len(p['fwd']) + ['d'] * len(p['dg'])
    gw = torch.zeros(weight.shape)
    ujobs = op.unpack_jobs(4, 4, gw)
    assert len(ujobs) == len(p['dg']) and all(j['masked'] is True and j['nslab'] == 1 and 'form' not in j for j in ujobs)
    assert [j['tap_off'] for j in ujobs] == words(p['dg'])
    for j, buf in zip(ujobs, p['dwp']):
        assert j['mmap'] is op.in_map and j['cmap'] is op.out_map and j['w'] is gw and j['packed'] is buf
        assert (j['Mp'], j['Cp'], j['s_m'], j['s_c']) == (op.Cip, op.Cop, 9, 7 * 9)
    with pytest.raises(NotImplementedError):
        op.pack(4, 4)


@pytest.mark.parametrize('mode, answers, nf, nd', [
    ('plain', {}, 1, 1),                                               # the 9-tap matrix of the whole concat, both forms
    ('segmented dgrad', {'segnb_conv_fprop_upd_ok': 1}, 1, 2),         # + skip's 9-tap and up's one 16-tap gather matrix
    ('segmented forward', {'segnb_upconv_fprop_acc_ok': 1}, 5, 1),     # skip's 9-tap matrix + up's four phase matrices
])
def test_upcat_pack_jobs_by_form(lib, monkeypatch, mode, answers, nf, nd):
    lib.answers.update(answers)
    monkeypatch.setattr(E.UpCatConvOp, 'segment_fwd', mode == 'segmented forward')
    rt = E.Runtime('cpu', 'bf16')
    op = E.UpCatConvOp(rt, torch.randn(40, 7, 3, 3), None, [(3, 8), (4, 8)])        # (40 outputs: above force_thin's 32)
    jobs = op.pack_jobs(16, 16, 2)
    assert [j['form'] for j in jobs].count('f') == nf and [j['form'] for j in jobs].count('d') == nd
    assert len(jobs) == nf + nd
    owners = {'f': [op.skip, op.up] if nf > 1 else [op.full], 'd': [op.skip, op.up] if nd > 1 else [op.full]}
    for f in 'fd':
        got = [j['packed'].data_ptr() for j in jobs if j['form'] == f]
        key = 'wp_fwd' if f == 'f' else 'wp_dg'
        assert got == [t.data_ptr() for o in owners[f] for t in o.plan(*((8, 8) if o is op.up else (16, 16)))[key]]
