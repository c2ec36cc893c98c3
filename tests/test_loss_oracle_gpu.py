"""The loss and metric kernels (csrc/head_loss.hip: segnb_seg_loss_*, segnb_pr_histogram, segnb_absmax_f32; csrc/mc_loss.hip)
on the MI355X against the float64 oracle of tests/loss_oracle.py, element by element under derived bounds, at saturation, at the
scalar tails and unaligned pointers, and across the inter-workgroup hand-overs (the one-launch binary form from 1 block to the
512-block cap and a second grid-stride trip; the multi-class row hand-over at 1, 15, 16, 17, 33 and 1024 workgroups).

The ABI is called directly through segnb._native, on the case list of tests/loss_cases.py; tests/test_loss_oracle_cpu.py runs
the same cases through fp32 CPU implementations and through their mutants."""
import pytest
import torch

import loss_cases as lc
import loss_oracle as lo
from segnb import _native as nv

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _named(prefix):
    return [c for c in lc.CASES if c[0].startswith(prefix)]


def _ids(cases):
    return [c[0] for c in cases]


@pytest.mark.parametrize('name,args', _named('binary-pixels'), ids=_ids(_named('binary-pixels')))
def test_binary_per_pixel_outputs(name, args):
    lc.run(DEV, args)


@pytest.mark.parametrize('name,args', _named('binary-reduce'), ids=_ids(_named('binary-reduce')))
def test_binary_one_launch_against_two_launch(name, args):
    lc.run(DEV, args)


@pytest.mark.parametrize('name,args', _named('binary-work') + _named('binary-halves') + _named('binary-degenerate'),
                         ids=_ids(_named('binary-work') + _named('binary-halves') + _named('binary-degenerate')))
def test_binary_work_buffer_halves_and_closed_forms(name, args):
    lc.run(DEV, args)


def test_one_launch_toggle_of_seglosses(monkeypatch):
    """segnb.seglosses with _ONE_LAUNCH on and off: both forms of the module path within the oracle's bound"""
    from segnb import seglosses as sl
    n = 524288 + 1029
    x, t = lo.binary_data(n, 9, '01')
    sp = lo.Spec(**lo.NAMED_SPECS['bce_smooth_jaccard'])
    F = lo.binary_fin(lo.binary_sums(x, t, sp.focal_gamma), sp)
    xd, td = x.to(DEV), t.to(DEV)
    for one in (True, False, True):
        monkeypatch.setattr(sl, '_ONE_LAUNCH', one)
        _, fin = sl.reduce_finalize(xd, td, sp.tuple())
        torch.cuda.synchronize()
        lo.check_fin(fin.cpu(), F, 'seglosses one_launch=%s' % one)
    for work in sl._loss_work.values():
        assert not bool(work.cpu().view(torch.int64).any())


@pytest.mark.parametrize('name,args', _named('mc-'), ids=_ids(_named('mc-')))
def test_multi_class(name, args):
    lc.run(DEV, args)


@pytest.mark.parametrize('name,args', _named('hist-'), ids=_ids(_named('hist-')))
def test_pr_histogram(name, args):
    lc.run(DEV, args)


@pytest.mark.parametrize('name,args', _named('absmax-'), ids=_ids(_named('absmax-')))
def test_absmax(name, args):
    lc.run(DEV, args)


def test_every_case_is_run():
    ran = sum(len(_named(p)) for p in ('binary-pixels', 'binary-reduce', 'binary-work', 'binary-halves', 'binary-degenerate', 'mc-',
                                       'hist-', 'absmax-'))
    assert ran == len(lc.CASES) and nv.has_test_backend() is False
