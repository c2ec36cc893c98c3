"""segnb.launchlist: the recording protocol against a fake of the three plan entry points.

Whichever way a recorded step ends, no recording stays open on the thread, the live handles are exactly those of the lists
still held, and segnb_plan_begin is never called while a recording is open."""
import pytest

from segnb import _native as nv
from segnb.launchlist import LaunchList, Recorder

from fake_plans import FakePlans, on_emulator


@pytest.fixture
def fake():
    yield _install(FakePlans())
    nv.set_backend_for_testing(None)


def _install(be):
    nv.set_backend_for_testing(be)
    return be


def _clean(be, held=()):
    return be.open == 0 and be.stray_ends == 0 and be.live == set(held)


def test_record_finish_replay_twice(fake):
    with Recorder() as rec:
        nv.call('launch')
        lst = rec.finish()
    assert lst and isinstance(lst, LaunchList) and lst.launches == 10
    assert _clean(fake, [100])
    seen = []
    lst.replay()
    lst.replay(seen.append)                   # no marks: `between` is never called
    assert fake.runs == [100, 100] and seen == []
    lst.destroy()
    assert _clean(fake)


def test_pauses_with_marks(fake):
    host = []
    with Recorder() as rec:
        with rec.pause('a'):                  # a mark known in advance
            assert fake.open == 0             # the host code runs outside the recording
            host.append(1)
        assert fake.open == 1
        with rec.pause() as seg:              # a mark known only behind the host code
            host.append(2)
            seg.mark = ('b', 2)
        lst = rec.finish()
    assert host == [1, 2] and lst.launches == 10 + 11 + 12 and _clean(fake, [100, 101, 102])
    for _ in range(2):
        order = []
        del fake.runs[:]
        lst.replay(lambda mark: order.append((mark, list(fake.runs))))
        # once per replay, in order, each behind the segment that ended at its cut; none behind the last segment
        assert order == [('a', [100]), (('b', 2), [100, 101])] and fake.runs == [100, 101, 102]
    lst.destroy()
    assert _clean(fake)


@pytest.mark.parametrize('exc', [RuntimeError, KeyboardInterrupt])
def test_host_code_raises_while_paused(fake, exc):
    state = []
    with pytest.raises(exc):
        with Recorder() as rec:
            with rec.pause('a'):
                pass
            try:
                with rec.pause('b'):
                    raise exc('hook')
            except BaseException:
                state.append(fake.open)       # the handler outside the pause finds the recording resumed
                raise
    assert state == [1] and fake.ended == 3 and _clean(fake)


@pytest.mark.parametrize('exc', [RuntimeError, KeyboardInterrupt])
def test_body_raises_while_recording(fake, exc):
    with pytest.raises(exc):
        with Recorder() as rec:
            with rec.pause('a'):
                pass
            raise exc('launch')
    assert fake.ended == 2 and _clean(fake)
    rec.abort()                               # idempotent: nothing is open, so nothing is ended
    assert fake.ended == 2 and _clean(fake)


@pytest.mark.parametrize('k', [0, 1, 2])
def test_refused_segment(k):
    be = _install(FakePlans(refuse=[k]))
    try:
        with Recorder() as rec:
            with rec.pause('a'):
                pass
            with rec.pause('b'):
                pass
            assert rec.finish() is None
        assert be.ended == 3 and _clean(be)
    finally:
        nv.set_backend_for_testing(None)


def test_block_left_without_finish_is_aborted(fake):
    with Recorder():
        nv.call('launch')
    assert _clean(fake)


def test_destroy_twice_and_del(fake):
    with Recorder() as rec:
        with rec.pause('a'):
            pass
        lst = rec.finish()
    kept = Recorder().finish()
    assert _clean(fake, [100, 101, 102])
    lst.destroy()
    lst.destroy()
    assert _clean(fake, [102])
    lst.__del__()                             # after destroy(): frees nothing twice (the fake answers an error if it did,
    del lst                                   # which __del__ would swallow: the live set is the judge)
    assert _clean(fake, [102])
    del kept                                  # a list dropped without destroy() frees its handles
    assert _clean(fake)


def _zf_unet_on_fake_lists(hook):
    """A small ZF_UNET on the ABI emulator, its recording path forced on (it is keyed to a GPU otherwise) with the fake's
    plan entry points; hook = the data-parallel "gradients ready" hook."""
    import torch
    from oracle import abi_emulator
    from lib.models.zf_unet import ZF_UNET
    fake = on_emulator(abi_emulator.AbiEmulator())
    torch.manual_seed(0)
    m = ZF_UNET(dropout_val=0.0, filters=4).set_compute_dtype('f32').train()
    m._grad_ready_hook = lambda flat, lo, producers: hook(fake, lo, producers)
    x = torch.randn(1, 3, 32, 32)
    with torch.no_grad():
        m(x)                                  # builds the engine
    eng = m._engine
    eng._cplan_key = lambda kind, *a: ('forced', kind) + tuple(str(v) for v in a[:3])
    return m, eng, fake, x


def _live_of(eng):
    return {seg.handle for p in eng._cplans.values() if p[0] for seg in p[0]._segments}


def test_zf_unet_cuts_its_backward_list_at_the_hook_and_replays_it():
    calls = []
    try:
        m, eng, fake, x = _zf_unet_on_fake_lists(lambda fake, lo, producers: calls.append((fake.open, lo, producers)))
        m(x).sum().backward()                 # recorded
        assert eng._rec is None and len(calls) == 2 and all(c[0] == 0 for c in calls)    # the hook ran outside the recording
        bwd = [p for k, p in eng._cplans.items() if k[1] == 'bwd']
        assert len(bwd) == 1 and bwd[0][0] and len(bwd[0][0]._segments) == 3 and bwd[0]['launches'] == bwd[0][0].launches
        assert _clean(fake, _live_of(eng)) and len(fake.live) == 4
        recorded, fake.runs = list(calls), []
        del calls[:]
        m.zero_grad()
        m(x).sum().backward()                 # replayed: every segment once, in order, the hook behind the first two
        assert fake.runs == sorted(fake.live) and calls == recorded and fake.ended == 4
        del bwd
        eng._cplans.clear()
        assert _clean(fake)                   # a list dropped by its owner frees its handles
    finally:
        nv.set_backend_for_testing(None)


@pytest.mark.parametrize('exc', [RuntimeError, KeyboardInterrupt])
def test_zf_unet_hook_raising_in_a_recorded_backward(exc):
    def hook(fake, lo, producers):
        raise exc('hook')
    try:
        m, eng, fake, x = _zf_unet_on_fake_lists(hook)
        with pytest.raises(exc):
            m(x).sum().backward()
        assert eng._rec is None and _clean(fake, _live_of(eng)) and len(fake.live) == 1      # the forward's list
        assert [p[0] for k, p in eng._cplans.items() if k[1] == 'bwd'] == [None]                  # remembered as eager
    finally:
        nv.set_backend_for_testing(None)


def _unet16_on_fake_lists(hook):
    """The same for an executor model (segnb.net.HipNet): the first step of a key is eager, the second one is recorded."""
    import torch
    from oracle import abi_emulator
    from lib.models.unet16 import UNet16
    fake = on_emulator(abi_emulator.AbiEmulator())
    torch.manual_seed(0)
    m = UNet16(num_filters=4).set_compute_dtype('f32').train()
    m._grad_ready_hook = lambda flat, lo, producers: hook(fake, lo, producers)
    m._plan_key = lambda x, need_grad, grads_alias: ('forced', tuple(x.shape), need_grad)
    x = torch.randn(1, 3, 32, 32)

    def step():
        m.zero_grad()
        m(x).sum().backward()
    return m, fake, step


def test_executor_model_pauses_for_unpack_and_hook_and_replays_both():
    calls = []
    try:
        m, fake, step = _unet16_on_fake_lists(lambda fake, lo, producers: calls.append((fake.open, lo, len(producers))))
        step()                                # eager (learns where the backward is cut)
        assert fake.ended == 0
        step()                                # recorded
        ent, = m._tape.plans.values()
        cuts = len(calls)
        assert cuts >= 1 and all(c[0] == 0 for c in calls)                  # the hook ran outside the recording
        assert ent['state'] == 'ready' and ent['nfwd'] == ent['fwd'].launches and ent['nbwd'] == ent['bwd'].launches
        assert len(ent['bwd']._segments) == cuts + 1
        assert _clean(fake, [s.handle for s in ent['fwd']._segments + ent['bwd']._segments])
        recorded, fake.runs = list(calls), []
        del calls[:]
        step()                                # replayed
        assert fake.runs == sorted(fake.live) and calls == recorded and fake.ended == cuts + 2
    finally:
        nv.set_backend_for_testing(None)


@pytest.mark.parametrize('exc', [RuntimeError, KeyboardInterrupt])
def test_executor_model_hook_raising_in_a_recorded_backward(exc):
    armed = []

    def hook(fake, lo, producers):
        if armed:
            raise exc('hook')
    try:
        m, fake, step = _unet16_on_fake_lists(hook)
        step()
        armed.append(1)
        with pytest.raises(exc):
            step()
        ent, = m._tape.plans.values()
        assert ent['state'] == 'eager' and 'fwd' not in ent and 'bwd' not in ent and _clean(fake)
        del armed[:]
        step()                                # the key is remembered as eager and still runs
        assert _clean(fake) and fake.runs == []
    finally:
        nv.set_backend_for_testing(None)
