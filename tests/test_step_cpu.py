"""segnb.step.StepCache alone, against the fake of the plan entry points (tests/fake_plans.py), and the guard bracket
(segnb.engine.ReplayGuard.step) on a fake census.  No model: the rule "however a recorded step ends, the entry is either
replayable or eager for good with nothing open and nothing live" is the cache's, not its owners'."""
import pytest

from segnb import _native as nv
from segnb.engine import ReplayGuard
from segnb.step import Entry, StepCache

from fake_plans import FakePlans


@pytest.fixture
def fake():
    be = FakePlans()
    nv.set_backend_for_testing(be)
    yield be
    nv.set_backend_for_testing(None)


def _clean(be, held=()):
    return be.open == 0 and be.stray_ends == 0 and be.live == set(held)


def _record(cache, ent, kind, body=lambda rec: None, store=True):
    with cache.recording(ent, kind) as rec:
        nv.call('launch')
        body(rec)
        if store:
            ent[kind] = rec.finish()
            if ent[kind]:
                ent['state'] = 'fwd' if kind == 'fwd' else 'ready'


def test_record_replay_destroy(fake):
    cache = StepCache()
    ent = cache.entry('k')
    assert cache.entry('k') is ent and ent['state'] == 'new' and ent[0] is None
    _record(cache, ent, 'fwd')
    _record(cache, ent, 'bwd')
    assert ent['state'] == 'ready' and ent[0] is ent['fwd'] and _clean(fake, [100, 101])
    ent['fwd'].replay()
    ent['bwd'].replay()
    assert fake.runs == [100, 101]
    ent.drop()
    assert _clean(fake) and 'fwd' not in ent and 'bwd' not in ent and ent[0] is None
    _record(cache, cache.entry('other'), 'fwd')
    cache.clear()                             # a cache emptied by its owner frees what its entries hold
    assert _clean(fake)


@pytest.mark.parametrize('exc', [RuntimeError, KeyboardInterrupt])
@pytest.mark.parametrize('paused', [False, True])
def test_body_that_raises_leaves_the_entry_eager_for_good(fake, exc, paused):
    cache = StepCache()
    ent = cache.entry('k')
    _record(cache, ent, 'fwd')

    def body(rec):
        with rec.pause('cut'):
            if paused:
                raise exc('hook')
        raise exc('launch')
    with pytest.raises(exc):
        _record(cache, ent, 'bwd', body)
    assert ent['state'] == 'eager' and ent[0] is None and 'fwd' not in ent and _clean(fake)      # the forward's list went too
    begun = fake.ended
    with cache.recording(ent, 'bwd') as rec:
        assert rec is None and fake.open == 0
    assert fake.ended == begun and _clean(fake)


@pytest.mark.parametrize('k', [0, 1])
def test_refused_segment_leaves_the_entry_eager_for_good(k):
    fake = FakePlans(refuse=[k])
    nv.set_backend_for_testing(fake)
    try:
        cache = StepCache()
        ent = cache.entry('k')

        def body(rec):
            with rec.pause('cut'):
                pass
        _record(cache, ent, 'fwd', body)
        assert ent['state'] == 'eager' and ent[0] is None and fake.ended == 2 and _clean(fake)
        fake.segnb_plan_begin = lambda: pytest.fail('segnb_plan_begin for an entry that is eager for good')
        for kind in ('fwd', 'bwd'):
            with cache.recording(ent, kind) as rec:
                assert rec is None
        assert _clean(fake)
    finally:
        nv.set_backend_for_testing(None)


def test_declined_list_leaves_the_entry_eager_for_good(fake):
    """the body finishes but keeps no list (the executor's `unplannable`)"""
    cache = StepCache()
    ent = cache.entry('k')
    _record(cache, ent, 'fwd')
    with cache.recording(ent, 'bwd') as rec:
        rec.finish().destroy()
    assert ent['state'] == 'eager' and ent[0] is None and _clean(fake)
    with cache.recording(ent, 'bwd') as rec:
        assert rec is None
    _record(cache, cache.entry('k2'), 'fwd', store=False)       # nor a body that never finishes its recording
    assert cache['k2']['state'] == 'eager' and _clean(fake)


def test_dropping_an_entry_that_holds_a_forward_list_only(fake):
    cache = StepCache()
    ent = cache.entry('k')
    _record(cache, ent, 'fwd')
    assert ent['state'] == 'fwd' and _clean(fake, [100])
    ent.drop()                                # (the executor: a recorded forward whose backward never ran)
    assert ent['state'] == 'fwd' and 'fwd' not in ent and _clean(fake)
    _record(cache, ent, 'fwd')                # ... is recorded again
    assert ent[0] is ent['fwd'] and _clean(fake, [101])
    with cache.recording(None, 'fwd') as rec:                  # no entry (no key): the body just runs
        assert rec is None and fake.open == 0


def test_bench_facing_views_in_every_state(fake):
    """bench.py: any(p[0] for p in model._engine._cplans.values()); any(e.get('state') == 'ready' for e in model._tape.plans.values())"""
    cache = StepCache()
    ent = cache.entry('k')
    seen = [(ent.get('state'), bool(ent[0]))]
    ent['state'] = 'seen'
    seen.append((ent.get('state'), bool(ent[0])))
    _record(cache, ent, 'fwd')
    seen.append((ent.get('state'), bool(ent[0])))
    _record(cache, ent, 'bwd')
    seen.append((ent.get('state'), bool(ent[0])))
    assert any(p[0] for p in cache.values()) and any(e.get('state') == 'ready' for e in cache.values())

    def boom(rec):
        raise RuntimeError('boom')
    ent.drop()
    with pytest.raises(RuntimeError):
        _record(cache, ent, 'bwd', boom)
    seen.append((ent.get('state'), bool(ent[0])))
    assert seen == [('new', False), ('seen', False), ('fwd', True), ('ready', True), ('eager', False)]
    assert not any(p[0] for p in cache.values()) and not any(e.get('state') == 'ready' for e in cache.values())
    bwd_only = cache.entry('zf bwd')          # ZF_UNET keeps the backward under a key of its own
    _record(cache, bwd_only, 'bwd')
    assert bwd_only[0] is bwd_only['bwd'] and isinstance(bwd_only, Entry) and _clean(fake, [103])


def test_guard_bracket_on_a_fake_census(monkeypatch):
    census = {}
    monkeypatch.setattr(nv, 'census_read', lambda: dict(census))
    monkeypatch.setattr(nv, 'has_test_backend', lambda: False)
    monkeypatch.setattr(nv, 'call', lambda name, *a: None)        # (segnb_tune "call_census")
    monkeypatch.setattr(ReplayGuard, 'enabled', True)
    monkeypatch.setattr(ReplayGuard, '_on', False)
    g = ReplayGuard('fake step')

    def step(mode, calls, raises=None, key='k'):
        with g.step() as s:
            s.begin()
            census.clear()
            census.update(calls, segnb_tune=1)
            s.key, s.mode = key, mode
            if raises:
                raise raises('boom')
    step('record', {'a': 2, 'b': 1})
    assert g.ref == {'k': {'a': 2, 'b': 1}} and g.checked == 0
    step('replay', {'a': 2, 'b': 1})
    assert g.checked == 1
    with pytest.raises(RuntimeError, match='replayed step does not execute.*b: recorded step 1, replayed step 0'):
        step('replay', {'a': 2})
    for exc in (RuntimeError, KeyboardInterrupt):
        with pytest.raises(exc, match='boom'):
            step('replay', {'a': 3}, raises=exc)                      # a step that raises is not compared ...
        with pytest.raises(exc, match='boom'):
            step('record', {'a': 3}, raises=exc)                      # ... and stores nothing
    assert g.ref == {'k': {'a': 2, 'b': 1}} and g.checked == 1
    step(None, {'a': 5})                                              # an eager step says neither
    with g.step():
        pass                                                          # nor does one that never reaches the list look-up
    step('replay', {'a': 9}, key='never recorded')
    assert g.checked == 1
    monkeypatch.setattr(ReplayGuard, 'enabled', False)
    step('replay', {'a': 9})                                          # guard off: nothing is read
    assert g.checked == 1
