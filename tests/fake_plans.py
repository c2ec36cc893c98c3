"""A fake of the plan entry points (segnb_plan_*), for the tests of the recording protocol and tools/abi_call_trace.py."""
from segnb import _native as nv


class FakePlans(object):
    """Hands out numbered handles; answers NULL for the segments (0-based, in the order they end) listed in `refuse`."""

    def __init__(self, refuse=()):
        self.refuse = set(refuse)
        self.open, self.ended, self.stray_ends, self.live, self.runs = 0, 0, 0, set(), []

    def segnb_plan_begin(self):
        assert self.open == 0, 'segnb_plan_begin while a recording is open'
        self.open += 1
        return 0

    def segnb_plan_end(self, handle_out, nops_out):
        if self.open == 0:
            self.stray_ends += 1              # (nv.plan_record_abort swallows this error: counted, _clean is the judge)
            return 1                          # "no plan is being recorded"
        self.open -= 1
        k, self.ended = self.ended, self.ended + 1
        nops_out._obj.value = 10 + k
        if k in self.refuse:
            handle_out._obj.value = None
        else:
            handle_out._obj.value = 100 + k
            self.live.add(100 + k)
        return 0

    def segnb_plan_run(self, handle):
        if handle not in self.live or self.open:
            return 1
        self.runs.append(handle)
        return 0

    def segnb_plan_destroy(self, handle):
        if handle not in self.live:
            return 1                          # freed twice, or never handed out
        self.live.remove(handle)
        return 0

    def launch(self):
        """stands for any recordable ABI call of the step"""
        return 0


def on_emulator(be, refuse=()):
    """Install the ABI emulator `be` with a fake's plan entry points grafted on.  -> the fake"""
    fake = FakePlans(refuse)
    for name in ('segnb_plan_begin', 'segnb_plan_end', 'segnb_plan_run', 'segnb_plan_destroy'):
        setattr(be, name, getattr(fake, name))
    nv.set_backend_for_testing(be)
    return fake
