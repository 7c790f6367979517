"""Launch hook for the schedule tests: every kernel of the step goes through `_lib.call`, and `engine.py`,
`trainer.py`, `jobs.py` and `losses.py` reach it as the module attribute `L.call`, so replacing that attribute (and
putting it back) reaches every launch.  Host code only: torch is touched when a default is first needed, never at import.

Modes
  log     record (index, entry point, stream handle, capturing?) per call; every mode keeps this log
  serial  after every call a device-wide synchronisation: the step with nothing overlapping at all.  Issue order is
          a legal schedule of a correct program (an event is recorded before it is waited on), so this is what the
          program means.  Eager only: a call made while a stream is capturing raises instead of synchronising
  delay   immediately before call number k, one spin kernel of `cycles` on the current stream: call k and everything
          behind it on that stream are held back while the other stream runs on into whatever it has queued.
          scope="capture": k counts the calls made while a stream is capturing only (the warm-up steps of a capture are
          not counted, the sleep becomes a kernel node of the captured branch)
"""
import contextlib
from collections import namedtuple

Launch = namedtuple("Launch", "index name stream capturing")

MODES = ("log", "serial", "delay")


def _torch_stream_id():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _torch_capturing():
    import torch
    return bool(torch.cuda.is_current_stream_capturing())


def _torch_sleep(cycles):
    import torch
    torch.cuda._sleep(int(cycles))


def _torch_sync():
    import torch
    torch.cuda.synchronize()


class LaunchHook:
    def __init__(self, mode="log", k=None, cycles=0, scope="all", sleep=None, sync=None, stream_id=None, capturing=None):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}")
        if scope not in ("all", "capture"):
            raise ValueError("scope must be 'all' or 'capture'")
        if mode == "delay" and (k is None or int(k) < 0 or int(cycles) <= 0):
            raise ValueError("delay mode needs a call index k >= 0 and cycles > 0")
        self.mode, self.k, self.cycles, self.scope = mode, (None if k is None else int(k)), int(cycles), scope
        self._sleep = sleep or _torch_sleep
        self._sync = sync or _torch_sync
        self._stream_id = stream_id or _torch_stream_id
        self._capturing = capturing or _torch_capturing
        self.log = []
        self.slept = []            # indices (of self.log) in front of which a sleep was enqueued
        self._scoped = 0           # calls counted towards k so far

    def names(self):
        return [e.name for e in self.log]

    def captured(self):
        """The calls made while a stream was capturing, re-indexed from 0 (the index that scope='capture' counts)."""
        caps = [e for e in self.log if e.capturing]
        return [Launch(i, e.name, e.stream, True) for i, e in enumerate(caps)]

    def wrap(self, call):
        def hooked(name, *args):
            cap = self._capturing()
            counted = cap or self.scope == "all"
            if self.mode == "delay" and counted and self._scoped == self.k:
                self._sleep(self.cycles)
                self.slept.append(len(self.log))
            if counted:
                self._scoped += 1
            self.log.append(Launch(len(self.log), name, self._stream_id(), cap))
            if self.mode == "serial" and cap:
                raise RuntimeError("serial mode synchronises the device after every call: not while a stream is capturing")
            out = call(name, *args)
            if self.mode == "serial":
                self._sync()
            return out
        return hooked


@contextlib.contextmanager
def installed(hook, module, attr="call"):
    """`module.attr` goes through `hook` inside the block; the original is back afterwards, whatever happened."""
    orig = getattr(module, attr)
    setattr(module, attr, hook.wrap(orig))
    try:
        yield hook
    finally:
        setattr(module, attr, orig)


def switch_points(log):
    """Indices where the stream differs from the previous call's, and the index just before each: the forks, joins
    and tail hand-offs of a log.  Sorted, without duplicates."""
    out = set()
    for i in range(1, len(log)):
        if log[i].stream != log[i - 1].stream:
            out.update((i - 1, i))
    return sorted(out)


def cover(n, groups):
    """`groups` contiguous ranges that partition range(n); their sizes differ by at most one (the later ones may be empty)."""
    if n < 0 or groups < 1:
        raise ValueError("cover(n, groups) needs n >= 0 and groups >= 1")
    q, r = divmod(n, groups)
    out, lo = [], 0
    for g in range(groups):
        hi = lo + q + (1 if g < r else 0)
        out.append(range(lo, hi))
        lo = hi
    return out
