"""The launch hook of the schedule tests (tests/_schedule.py) against a fake `call` and a fake sleep: no GPU."""
import types

import pytest

from _schedule import LaunchHook, Launch, cover, installed, switch_points


class _Fake:
    """A module-like object with a `call`, plus recorders standing in for the stream, the sleep and the sync."""

    def __init__(self, streams=None, capturing=None):
        self.events = []                  # ("call", name, args) / ("sleep", cycles) / ("sync",) in issue order
        self.streams = streams or {}      # call number -> stream handle (default 1)
        self.capturing = capturing or set()
        self.n = 0                        # calls the hook has asked about so far
        self.mod = types.SimpleNamespace(call=self._call)
        self.orig = self.mod.call

    def _call(self, name, *args):
        self.events.append(("call", name, args))
        if name == "refuse":
            raise ValueError("refuse: invalid argument")
        return ("ret", name)

    def kw(self):
        def capturing():
            return self.n in self.capturing

        def stream_id():
            s = self.streams.get(self.n, 1)
            self.n += 1
            return s
        return dict(sleep=lambda c: self.events.append(("sleep", c)), sync=lambda: self.events.append(("sync",)),
                    stream_id=stream_id, capturing=capturing)


def _run(fake, hook, names):
    with installed(hook, fake.mod):
        for i, n in enumerate(names):
            fake.mod.call(n, i, "x")
    return hook


def test_log_indices_are_dense_and_in_order():
    f = _Fake(streams={2: 7, 3: 7}, capturing={3})
    h = _run(f, LaunchHook("log", **f.kw()), ["a", "b", "c", "d", "e"])
    assert [e.index for e in h.log] == list(range(5))
    assert h.names() == ["a", "b", "c", "d", "e"]
    assert [e.stream for e in h.log] == [1, 1, 7, 7, 1]
    assert [e.capturing for e in h.log] == [False, False, False, True, False]
    assert f.events == [("call", n, (i, "x")) for i, n in enumerate("abcde")]      # nothing but the calls themselves
    assert h.slept == []


@pytest.mark.parametrize("k", [0, 2, 4])
def test_delay_sleeps_once_before_call_k_and_changes_nothing_else(k):
    names = ["a", "b", "c", "d", "e"]
    f = _Fake()
    h = _run(f, LaunchHook("delay", k=k, cycles=123, **f.kw()), names)
    want = [("call", n, (i, "x")) for i, n in enumerate(names)]
    want.insert(k, ("sleep", 123))
    assert f.events == want
    assert h.slept == [k] and h.names() == names


def test_delay_past_the_last_call_never_sleeps():
    f = _Fake()
    h = _run(f, LaunchHook("delay", k=9, cycles=5, **f.kw()), ["a", "b"])
    assert h.slept == [] and ("sleep", 5) not in f.events


def test_delay_in_capture_scope_counts_captured_calls_only():
    # calls 0-2 are a capture's eager warm-up, 3-6 the capture itself: k = 1 is the second captured call, log index 4
    f = _Fake(capturing={3, 4, 5, 6})
    h = _run(f, LaunchHook("delay", k=1, cycles=11, scope="capture", **f.kw()), list("abcdefg"))
    assert h.slept == [4]
    assert f.events.index(("sleep", 11)) == 4 and f.events[5][:2] == ("call", "e")
    assert [(e.index, e.name) for e in h.captured()] == [(0, "d"), (1, "e"), (2, "f"), (3, "g")]
    assert sum(e[0] == "sleep" for e in f.events) == 1


def test_serial_synchronises_after_every_call_and_refuses_a_capture():
    f = _Fake()
    _run(f, LaunchHook("serial", **f.kw()), ["a", "b"])
    assert f.events == [("call", "a", (0, "x")), ("sync",), ("call", "b", (1, "x")), ("sync",)]
    f = _Fake(capturing={1})
    with pytest.raises(RuntimeError, match="capturing"):
        _run(f, LaunchHook("serial", **f.kw()), ["a", "b", "c"])
    assert f.events == [("call", "a", (0, "x")), ("sync",)]        # neither the captured call nor a sync went out
    assert f.mod.call == f.orig


@pytest.mark.parametrize("mode", ["log", "serial", "delay"])
def test_arguments_results_and_exceptions_pass_through(mode):
    f = _Fake()
    h = LaunchHook(mode, k=1 if mode == "delay" else None, cycles=3, **f.kw())
    marker = object()
    with installed(h, f.mod):
        assert f.mod.call("a", marker, None, 2.5) == ("ret", "a")
        with pytest.raises(ValueError, match="refuse: invalid argument"):
            f.mod.call("refuse", marker)
        assert f.mod.call("b") == ("ret", "b")
    calls = [e for e in f.events if e[0] == "call"]
    assert calls[0][2] == (marker, None, 2.5) and calls[0][2][0] is marker
    assert calls[1] == ("call", "refuse", (marker,))
    assert h.names() == ["a", "refuse", "b"]                       # the refused call keeps its index


def test_original_call_is_restored_after_an_exception():
    f = _Fake()
    with pytest.raises(ValueError):
        with installed(LaunchHook("log", **f.kw()), f.mod):
            assert f.mod.call != f.orig
            f.mod.call("refuse")
    assert f.mod.call == f.orig
    with pytest.raises(KeyError):
        with installed(LaunchHook("log", **f.kw()), f.mod):
            raise KeyError("from the block itself")
    assert f.mod.call == f.orig


def test_bad_arguments_are_refused():
    with pytest.raises(ValueError):
        LaunchHook("sometimes")
    with pytest.raises(ValueError):
        LaunchHook("delay")                       # no k
    with pytest.raises(ValueError):
        LaunchHook("delay", k=2, cycles=0)
    with pytest.raises(ValueError):
        LaunchHook("log", scope="graph")


def _log(streams):
    return [Launch(i, f"k{i}", s, False) for i, s in enumerate(streams)]


def test_switch_points_on_hand_written_logs():
    assert switch_points([]) == [] and switch_points(_log([1])) == [] and switch_points(_log([1, 1, 1])) == []
    # fork after call 1, join before call 4
    assert switch_points(_log([1, 1, 2, 2, 1, 1])) == [1, 2, 3, 4]
    # a single side launch: both of its neighbours and itself, no duplicates
    assert switch_points(_log([1, 2, 1])) == [0, 1, 2]
    # a switch at the very end and three streams
    assert switch_points(_log([1, 1, 1, 2])) == [2, 3]
    assert switch_points(_log([1, 2, 2, 2, 3, 3, 1])) == [0, 1, 3, 4, 5, 6]


@pytest.mark.parametrize("n,groups", [(0, 1), (0, 4), (1, 4), (3, 4), (4, 4), (5, 4), (97, 6), (128, 1), (131, 8)])
def test_cover_is_a_partition(n, groups):
    parts = cover(n, groups)
    assert len(parts) == groups
    flat = [i for p in parts for i in p]
    assert flat == list(range(n))                              # every index once, in order: disjoint and complete
    sizes = [len(p) for p in parts]
    assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        cover(n, 0)
