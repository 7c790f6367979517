"""The step's results are a function of issue order, not of timing.

engine.py runs the training step on two streams (the pair term and the decoder's weight gradients with their
reductions, the loss bookkeeping, and the side-stream tail ride a side stream); both streams use persistent temporaries
at fixed addresses, and every step reuses the buffers of the one before.  Correctness rests on the events, waits and
joins between them: a missing edge is a stale read or an overwrite under a reader -- at one lucky timing invisible.
Here the timing is made adversarial.  Every launch goes through `_lib.call`; a hook (tests/_schedule.py) holds ONE
launch back with a spin kernel on its own stream, long enough for the other stream to drain everything it has queued,
and the results of two consecutive optimiser steps (losses, gradients, parameters) must stay bit for bit what they are
when nothing overlaps at all (a device-wide synchronisation after every launch: issue order, which is always a legal
schedule of a correct program).  Every launch index of the two steps is delayed in some run, per configuration; the
captured graph gets the sleep as a kernel node of the branch at every stream switch; the autograd route through
Seq2SeqBinaryVAE.__call__ + backward() is walked over its switch points and their neighbours; and with the side
tail's wait for the BPTT launch made a no-op the same comparison must FAIL (the harness can see a missing edge).

Persistent temporaries never hold the right answer by accident: a first step runs on a third batch, every run's
step 1 finds the buffers of the previous run's step 2 (another batch, other weights) and step 2 those of step 1.

No tolerance anywhere: every comparison is torch.equal on int32 bit patterns.

Measured on one MI355X (every test prints its own figures, `-s`):
  configuration      launches/step  streams  stream switches (two-step log)          two steps   _sleep(1e7)  cycles
  percep_f32_eval         35           2     10-12 23|24 32|33 (+35 in step 2)        1.743 ms    5.308 ms    13 133 202
  percep_bf16_train       31           2      8-10 19|20 28|29 (+31)                  1.706 ms    4.180 ms    16 326 725
  triplet_f32_eval        36           2     10-13 24|25 33|34 (+36)                  1.740 ms    4.168 ms    16 702 241
  autograd route          34           2     23|24 32|33 (+34), backward only         4.890 ms    4.170 ms    46 901 203
  (the process's first _sleep(1e7) took 5.3 ms, the later ones 4.2: the margin of 4 covers such drift)
  delayed runs compared: 70 + 62 + 72 eager (every index), 7 captures of the 31-node graph (one per switch point and
  its predecessor), 15 on the autograd route: 226 runs, 0 differ.  With the side tail's wait for ev_bptt dropped and
  rbvae_lstm_pair_bwd (call 17) delayed: differs from step 1's encoder_rnn.lstm.weight_ih_l0[0] on; restored: equal.
  Run time per test: 0.12-0.23 s per group of 15-18 delayed runs, 0.14 s the graph leg, 0.65 s the autograd route,
  0.71 s the first test (it builds the first trainer); the module 5.2 s.
"""
import math
import sys
from importlib import import_module

import pytest
import torch

from _schedule import LaunchHook, cover, installed, switch_points

pytestmark = pytest.mark.gpu

B, T, LD, HW = 2, 3, 32, (16, 16)         # test_trainer_gpu.py's smallest: four-layer stacks, paired BPTT, side tail
TAU = 0.8
GROUPS = 4                                # delayed runs of one configuration are spread over this many tests
MARGIN = 4                                # the sleep lasts at least this many two-step durations (stimulus, not a gate)
CONFIGS = {
    "percep_f32_eval": dict(variant="percep", in_ch=4, dtype="f32", train=False, device_noise=False),
    "percep_bf16_train": dict(variant="percep", in_ch=4, dtype="bf16", train=True, device_noise=True),   # the benched path
    "triplet_f32_eval": dict(variant="triplet", in_ch=3, dtype="f32", train=False, device_noise=False),
}
BPTT = ("rbvae_lstm_pair_bwd", "rbvae_lstm_bwd", "rbvae_lstm_bwd_ex", "rbvae_lstm_bwd_bin")


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _first_diff(a, b):
    x, y = _bits(a).reshape(-1), _bits(b).reshape(-1)
    if torch.equal(x, y):
        return None
    return int((x != y).nonzero()[0])


def _param_at(lay, i):
    for n in lay.names:
        o = lay.offsets[n]
        if o <= i < o + math.prod(lay.shapes[n]):
            return f"{n}[{i - o}]"
    return f"padding[{i}]"


def _sleep_cycles(run_two_steps):
    """Cycles for which torch.cuda._sleep lasts MARGIN times the unperturbed eager two-step run: both measured here,
    with events, on this device at its present clocks."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    two = 0.0
    for _ in range(2):
        torch.cuda.synchronize()
        ev[0].record()
        run_two_steps()
        ev[1].record()
        torch.cuda.synchronize()
        two = max(two, ev[0].elapsed_time(ev[1]))
    ev[2].record()
    torch.cuda._sleep(10 ** 7)
    ev[3].record()
    torch.cuda.synchronize()
    sleep = ev[2].elapsed_time(ev[3])
    assert two > 0.0 and sleep > 0.0, (two, sleep)
    cycles = int(math.ceil(MARGIN * two / sleep * 10 ** 7))
    return cycles, two, sleep


class _Phases:
    """Marks which slice of a hook's log each engine.forward / engine.backward call issued."""

    def __init__(self, eng, hook):
        self.eng, self.hook, self.spans = eng, hook, []

    def __enter__(self):
        for what in ("forward", "backward"):
            inner = getattr(self.eng, what)

            def outer(*a, _inner=inner, _what=what, **kw):
                lo = len(self.hook.log)
                try:
                    return _inner(*a, **kw)
                finally:
                    self.spans.append((_what, lo, len(self.hook.log)))
            setattr(self.eng, what, outer)
        return self

    def __exit__(self, *exc):
        for what in ("forward", "backward"):
            delattr(self.eng, what)             # the instance attribute: the class's method shows again

    def switches(self, what):
        log = self.hook.log
        return [i for w, lo, hi in self.spans if w == what for i in range(lo + 1, hi) if log[i].stream != log[i - 1].stream]


class _Trainer:
    """One configuration: trainer, state snapshot, serial reference, launch log, sleep length.  Built once per module run
    and left unchanged; every run restores the snapshot first."""

    def __init__(self, name):
        cfg = CONFIGS[name]
        import sfv_amd as sfv
        self.name = name
        self.L = import_module("symbols-from-video_amd._lib")
        FT = import_module("symbols-from-video_amd.trainer").FusedTrainer
        torch.manual_seed(71)
        m = sfv.Seq2SeqBinaryVAE(cfg["in_ch"], cfg["in_ch"], LD, LD, variant=cfg["variant"], input_hw=HW,
                                 compute_dtype=cfg["dtype"]).cuda()
        m.train(cfg["train"])
        g = torch.Generator().manual_seed(72)
        self.items = [torch.rand(B, 2, T, cfg["in_ch"], *HW, generator=g).cuda() for _ in range(3)]
        self.U = [None if cfg["device_noise"] else torch.rand(2, B * T, LD, generator=g).cuda() for _ in range(3)]
        self.m = m
        self.tr = tr = FT(m, lr=1e-3, alpha=1.0, beta_kl=0.5, bernoulli_p=0.1, noise_ratio=0.1, margin=0.2,
                          device_noise=cfg["device_noise"], use_graph=False, seed=7)
        # warm-up step on a THIRD batch: engine, tables and side stream exist, Adam's moments are not zero, and the
        # persistent temporaries hold plausible values that belong to neither step below
        tr.step(self.items[0], TAU, U=self.U[0])
        torch.cuda.synchronize()
        self.snap = (m._flat.clone(), tr.m.clone(), tr.vv.clone(), tr.step_dev.clone(), tr.steps)
        self.lay = tr.eng.layout
        # reference: the two steps with nothing overlapping at all
        self.ref, _ = self.run(LaunchHook("serial"))
        # log of one unperturbed run
        hook = LaunchHook("log")
        with _Phases(tr.eng, hook) as ph:
            self.plain, _ = self.run(hook)
        self.log, self.phases = hook.log, ph
        self.n = len(self.log)
        self.cycles, self.two_ms, self.sleep_ms = _sleep_cycles(lambda: (self.restore(), self.two_steps()))
        print(f"\n{name}: {self.n} launches in two steps ({self.n // 2} per step) on {len({e.stream for e in self.log})} "
              f"streams, switch points {switch_points(self.log)}; eager two-step run {self.two_ms:.3f} ms, "
              f"_sleep(1e7) {self.sleep_ms:.3f} ms -> cycles {self.cycles} (>= {MARGIN} x the run)")

    def restore(self):
        flat0, m0, v0, s0, steps = self.snap
        tr = self.tr
        self.m._flat.copy_(flat0)
        tr.m.copy_(m0)
        tr.vv.copy_(v0)
        tr.step_dev.copy_(s0)                # Adam's step count (and the key of the device-side noise) equal across runs
        tr.steps = steps
        tr.eng.pack(self.m._flat)

    def two_steps(self):
        out = []
        for i in (1, 2):
            losses = self.tr.step(self.items[i], TAU, U=self.U[i])
            # stream-ordered copies on the main stream, behind the step's update launch: no host synchronisation here
            out.append((losses.clone(), self.tr.gflat.clone(), self.m._flat.clone()))
        return out

    def run(self, hook):
        self.restore()
        torch.cuda.synchronize()
        with installed(hook, self.L):
            out = self.two_steps()
        torch.cuda.synchronize()
        return out, hook

    def differences(self, got, ref=None):
        """[(step, what, first differing element)] between two runs' results."""
        out = []
        for s, (g, r) in enumerate(zip(got, self.ref if ref is None else ref)):
            for what, a, b in zip(("losses", "gflat", "parameters"), g, r):
                i = _first_diff(a, b)
                if i is not None:
                    out.append((s + 1, what, i if what == "losses" else _param_at(self.lay, i)))
        return out

    def check(self, got, hook, k):
        d = self.differences(got)
        e = hook.log[hook.slept[0]] if hook.slept else None
        assert not d, (f"{self.name}: delaying call {k} ({e.name if e else '?'}, stream {e.stream if e else '?'}, "
                       f"{self.cycles} cycles) changed the results; first differences (step, what, element): {d[:6]}")


_CACHE = {}


def _ctx(name):
    if name not in _CACHE:
        _CACHE[name] = _Trainer(name)
    return _CACHE[name]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_unperturbed_steps_repeat_and_equal_the_serial_reference(name):
    """Precondition: two unperturbed eager runs from the snapshot are bit-identical (else nothing below means
    anything), and they are what the serial reference computes."""
    c = _ctx(name)
    again, hook = c.run(LaunchHook("log"))
    assert hook.names() == [e.name for e in c.log]
    assert all(torch.isfinite(x).all() for step in c.ref for x in step)
    assert not c.differences(again, c.plain), ("two unperturbed runs differ", c.differences(again, c.plain)[:6])
    assert not c.differences(c.plain), ("unperturbed differs from serial", c.differences(c.plain)[:6])
    # and the two steps are different problems: a stale read of the other step's buffers cannot go unnoticed
    assert c.differences([c.ref[0]], [c.ref[1]])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_log_shows_side_stream_work_in_forward_and_backward(name):
    c = _ctx(name)
    assert len({e.stream for e in c.log}) >= 2
    assert not any(e.capturing for e in c.log)
    assert [w for w, _, _ in c.phases.spans] == ["forward", "backward"] * 2
    assert c.phases.switches("forward") and c.phases.switches("backward"), c.phases.spans
    assert any(e.name in BPTT for e in c.log)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_groups_cover_every_launch_index(name):
    c = _ctx(name)
    parts = cover(c.n, GROUPS)
    assert c.n > 0 and sorted(i for p in parts for i in p) == list(range(c.n))


@pytest.mark.parametrize("group", range(GROUPS))
@pytest.mark.parametrize("name", list(CONFIGS))
def test_delayed_launch_leaves_both_steps_bit_equal(name, group):
    c = _ctx(name)
    names = [e.name for e in c.log]
    ks = cover(c.n, GROUPS)[group]
    for k in ks:
        got, hook = c.run(LaunchHook("delay", k=k, cycles=c.cycles))
        assert hook.slept == [k] and hook.names() == names          # the sleep went out, in front of the same launch
        c.check(got, hook, k)
    print(f"\n{name} group {group}: calls {ks.start}..{ks.stop - 1} delayed one at a time, 0 of {len(ks)} runs differ")


def test_graph_replay_with_a_sleep_node_at_every_stream_switch():
    """The benched path from its captured graph: the hook stays in delay mode while FusedTrainer._capture runs, so the
    sleep becomes a kernel node of the branch it was issued on; two replays against the eager serial reference."""
    c = _ctx("percep_bf16_train")
    tr = c.tr

    def run(hook):
        tr._graphs.clear()
        c.restore()
        torch.cuda.synchronize()
        with installed(hook, c.L):
            out = c.two_steps()
        torch.cuda.synchronize()
        return out

    tr.use_graph = True
    try:
        hook = LaunchHook("log")
        got = run(hook)
        cap = hook.captured()
        assert len(tr._graphs) == 1 and len(cap) == c.n // 2, (len(cap), c.n)
        assert [e.name for e in cap] == [e.name for e in c.log[:len(cap)]]
        assert len({e.stream for e in cap}) >= 2
        assert not c.differences(got), ("undelayed replay differs from the eager serial reference", c.differences(got)[:6])
        sp = switch_points(cap)
        assert 4 <= len(sp) <= 24, sp
        for k in sp:
            hook = LaunchHook("delay", k=k, cycles=c.cycles, scope="capture")
            got = run(hook)
            assert len(hook.slept) == 1 and hook.log[hook.slept[0]].capturing
            assert hook.captured()[k].name == hook.log[hook.slept[0]].name == cap[k].name
            c.check(got, hook, k)
        print(f"\ngraph leg: {len(cap)} kernel nodes, one capture per switch point {sp}, 0 of {len(sp)} differ")
    finally:
        tr.use_graph = False
        tr._graphs.clear()
        c.restore()
        torch.cuda.synchronize()


def test_autograd_route_is_timing_independent():
    """Seq2SeqBinaryVAE.__call__ + backward(): engine.forward / engine.backward without the trainer (no pair term, no
    bookkeeping: the decoder's weight gradients and the side tail).  Same protocol over its switch points +- 1."""
    import sfv_amd as sfv
    L = import_module("symbols-from-video_amd._lib")
    torch.manual_seed(81)
    m = sfv.Seq2SeqBinaryVAE(4, 4, LD, LD, variant="percep", input_hw=HW, compute_dtype="f32").cuda().eval()
    g = torch.Generator().manual_seed(82)
    xs = [torch.rand(B, T, 4, *HW, generator=g).cuda() for _ in range(3)]
    us = [torch.rand(B * T, LD, generator=g).cuda() for _ in range(3)]

    def one(i):
        m._seed = 0
        xr, hs, z = m(xs[i], temperature=TAU, hard=False, u=us[i])
        ((xr - xs[i]).square().mean() + 0.1 * hs.square().mean() + 0.5 * z.mean()).backward()
        return xr.detach().clone(), hs.detach().clone(), z.detach().clone(), m._gflat.clone()

    def run(hook):
        torch.cuda.synchronize()
        with installed(hook, L):
            out = [one(1), one(2)]
        torch.cuda.synchronize()
        return out

    def diffs(a, b):
        return [(s + 1, what, i) for s, (x, y) in enumerate(zip(a, b))
                for what, p, q in zip(("xr", "hs", "z", "gflat"), x, y) for i in [_first_diff(p, q)] if i is not None]

    one(0)                                               # warm-up on a third batch
    torch.cuda.synchronize()
    eng = next(iter(m._engines.values()))
    ref = run(LaunchHook("serial"))
    hook = LaunchHook("log")
    with _Phases(eng, hook) as ph:
        plain = run(hook)
    again = run(LaunchHook("log"))
    assert not diffs(plain, again) and not diffs(plain, ref), (diffs(plain, again)[:4], diffs(plain, ref)[:4])
    assert diffs([ref[0]], [ref[1]])
    log = hook.log
    assert len({e.stream for e in log}) >= 2 and ph.switches("backward")
    cycles, two_ms, sleep_ms = _sleep_cycles(lambda: (one(1), one(2)))
    sp = switch_points(log)
    ks = sorted({j for i in sp for j in (i - 1, i, i + 1) if 0 <= j < len(log)})
    for k in ks:
        h = LaunchHook("delay", k=k, cycles=cycles)
        got = run(h)
        assert h.slept == [k] and h.names() == [e.name for e in log]
        d = diffs(got, ref)
        assert not d, (f"autograd route: delaying call {k} ({log[k].name}, stream {log[k].stream}) changed the results; "
                       f"first differences (pass, what, element): "
                       f"{[(s, w, _param_at(eng.layout, i) if w == 'gflat' else i) for s, w, i in d[:6]]}")
    print(f"\nautograd route: {len(log)} launches in two passes, switch points {sp}; two passes {two_ms:.3f} ms, "
          f"_sleep(1e7) {sleep_ms:.3f} ms -> cycles {cycles}; {len(ks)} delayed runs, 0 differ")


def test_a_dropped_tail_wait_is_seen(monkeypatch):
    """Sensitivity: with the side tail's wait for the BPTT launch (ev_bptt: it guards the float buffers dG_dec / dG_enc
    that rbvae_lstm_wgrad_pair reads, nothing a kernel uses as an address) made a no-op in this process and the BPTT
    launch held back, the LSTM weight gradients are formed from the previous pass's dG: the results must differ."""
    c = _ctx("percep_f32_eval")
    k = next(e.index for e in c.log if e.name in BPTT)                # step 1's (first) BPTT launch: the producer
    orig = torch.cuda.Stream.wait_event
    tail_waits = []

    def wait_event(self, ev):
        # the direct wait_event calls of engine.backward's issue_decoder_side are the side tail's, ev_bptt first, ev_de
        # second in every pass (Stream.wait_stream's own call comes from another frame and goes through)
        if sys._getframe(1).f_code.co_name == "issue_decoder_side":
            tail_waits.append(ev)
            if len(tail_waits) % 2 == 1:
                return None
        return orig(self, ev)

    monkeypatch.setattr(torch.cuda.Stream, "wait_event", wait_event)
    try:
        got, hook = c.run(LaunchHook("delay", k=k, cycles=c.cycles))
    finally:
        monkeypatch.undo()
    assert torch.cuda.Stream.wait_event is orig
    assert len(tail_waits) == 4, len(tail_waits)                      # two per pass: the filter met what it was written for
    d = c.differences(got)
    assert d, f"the harness is blind: {hook.log[k].name} delayed with the tail's wait dropped and nothing differs"
    assert any(what == "gflat" and "rnn.lstm.weight" in str(el) for _, what, el in d), d[:6]
    # the wait restored, the same delay again: equal
    got, hook = c.run(LaunchHook("delay", k=k, cycles=c.cycles))
    c.check(got, hook, k)
    print(f"\nsensitivity: ev_bptt wait dropped, call {k} ({c.log[k].name}) delayed: differs at {d[:3]}; restored: equal")
