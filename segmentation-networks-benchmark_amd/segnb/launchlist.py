"""Recorded launch lists (segnb_plan_*: include/segnb_hip.h): the one place that speaks the recording protocol.

A step is launched once from Python while the library records the ABI calls of this thread (``Recorder``); later steps
replay the list from C (``LaunchList.replay``).  Host code that must run BETWEEN launches cuts the list into segments:
``Recorder.pause`` ends one, runs the caller outside the recording and leaves a *mark* that the replay hands to its
``between`` callback.  However a recorded step ends -- finished, refused by the library, left by an exception (also while
paused) -- no recording stays open on the thread and the only live handles are those of the LaunchList handed out."""
import contextlib
import types

from . import _native as nv


def _destroy(segments):
    """Every handle is tried; the first failure is raised behind the last one."""
    failed = None
    for seg in segments:
        if seg.handle is not None:
            handle, seg.handle = seg.handle, None
            try:
                nv.call('segnb_plan_destroy', handle)
            except Exception as e:
                failed = failed or e
    if failed is not None:
        raise failed


class LaunchList(object):
    """The replayable segments of one recorded step; owns their handles."""

    def __init__(self, segments):
        self._segments = segments
        self.launches = sum(seg.launches for seg in segments)

    def replay(self, between=None):
        """Run every segment; between(mark) is called behind a segment that carries a mark."""
        for seg in self._segments:
            nv.call('segnb_plan_run', seg.handle)
            if seg.mark is not None and between is not None:
                between(seg.mark)

    def destroy(self):
        segments, self._segments = self._segments, []
        _destroy(segments)

    def __del__(self):
        try:
            self.destroy()
        except Exception:          # (interpreter shutdown: the library may be gone already)
            pass


class Recorder(object):
    """Records the ABI calls of this thread from its construction to finish(); as a context manager it aborts when the body
    is left without one (any BaseException: an open recording swallows every later ABI call, e.g. of a Ctrl-C handler)."""

    def __init__(self):
        self._segments = []        # finished segments; the library refused those whose handle is None
        self._open = False
        self._begin()

    def _begin(self):
        assert not self._open
        nv.plan_record_begin()
        self._open = True

    def _end(self):
        self._open = False         # (segnb_plan_end fails only when nothing is being recorded)
        handle, launches = nv.plan_record_end()
        seg = types.SimpleNamespace(handle=handle, launches=launches, mark=None)
        self._segments.append(seg)     # owned here before any host code of the caller can raise
        return seg

    @contextlib.contextmanager
    def pause(self, mark=None):
        """The body runs OUTSIDE the recording; yields the segment that just ended (a mark known only behind the host code:
        ``seg.mark = ...``).  Resumes also when the body raises: the handler outside finds the state of any failed launch."""
        seg = self._end()
        seg.mark = mark
        try:
            yield seg
        finally:
            self._begin()

    def finish(self):
        """-> the LaunchList, or None when the library refused a segment (the others are destroyed then)."""
        self._end()
        segments, self._segments = self._segments, []
        if any(seg.handle is None for seg in segments):
            _destroy(segments)
            return None
        return LaunchList(segments)

    def abort(self):
        """Close the recording if one is open and free every finished segment."""
        if self._open:
            self._open = False
            nv.plan_record_abort()
        segments, self._segments = self._segments, []
        _destroy(segments)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self.abort()               # (nothing left to do behind finish())
        return False
