"""CPU: the host helpers the latent analyses share (_latents.py, and mixture.py's criteria and select): the labels of the
script's frames, model selection, and the driver of an iteration that is decided on the device, here driven by a state on
the host."""
import math
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sfv_amd as sfv

H = import_module("symbols-from-video_amd._latents")


def test_frame_labels():
    labels = H.frame_labels(range(40), [10, 30], 40)
    assert labels.dtype == np.int64 and labels.shape == (40,)
    for f in range(40):
        assert labels[f] == sfv.assign_label(f, [10, 30]), f
    assert sorted(set(labels.tolist())) == [0, 1, 2]
    with pytest.raises(ValueError, match="^39 frame indices for 40 frames$"):
        H.frame_labels(range(39), [10, 30], 40)


def test_frame_count_precedence_on_the_host():
    for x in (torch.zeros((2, 3, 8, 8)), np.zeros((2, 3, 8, 8)), None):
        with pytest.raises(ValueError, match=r"^x must be on the GPU \(there is no CPU path\)$"):
            H.frame_count(x)


def test_criteria():
    bic, aic = sfv.mixture.criteria(-1.25, 1500, 52)
    assert bic == -2.0 * -1.25 * 1500 + 52 * math.log(1500) and aic == -2.0 * -1.25 * 1500 + 2.0 * 52
    assert sfv.hmm_model._criteria(-1.25, 1500, 4, 3) == sfv.mixture.criteria(-1.25, 1500, sfv.hmm_model.n_parameters(4, 3))


def _select(ks, scores, criterion="bic"):
    X = np.zeros((100, 3), dtype=np.float32)
    fits = []

    def fit(K):
        fits.append(SimpleNamespace(K=K, n_iter=K + 1, converged=K % 2 == 0))
        return fits[-1]

    return sfv.mixture.select(X, ks, criterion, fit, lambda f: scores[f.K], lambda K, Ld: 0), fits


def test_select():
    (table, K, best), fits = _select((5, 3, 4), {5: -1.0, 3: -1.0, 4: -2.0})
    assert [r["K"] for r in table] == [5, 3, 4] and K == 3 and best is fits[1]        # a tie goes to the smaller K
    assert table[1] == {"K": 3, "n_iter": 4, "converged": False, "score": -1.0, "bic": 200.0, "aic": 200.0}
    (table, K, best), fits = _select((2, 3), {2: -1.0, 3: -0.5})
    assert K == 3 and best is fits[1] and table[0]["bic"] == 200.0 and table[1]["bic"] == 100.0
    # p = n_parameters(K, L) reaches both criteria: one parameter per component turns the order at N = 100
    X = np.zeros((100, 3), dtype=np.float32)
    fit = lambda K: SimpleNamespace(K=K, n_iter=1, converged=True)       # noqa: E731
    table, K, _ = sfv.mixture.select(X, (2, 40), "bic", fit, lambda f: -1.0 + 0.005 * f.K, lambda K, Ld: K * Ld)
    assert K == 2 and table[1]["bic"] == -2.0 * (-1.0 + 0.005 * 40) * 100 + 120 * math.log(100)
    assert sfv.mixture.select(X, (2, 40), "aic", fit, lambda f: -1.0 + 0.02 * f.K, lambda K, Ld: K * Ld)[1] == 2
    assert sfv.mixture.select(X, (2, 40), "aic", fit, lambda f: -1.0 + 0.04 * f.K, lambda K, Ld: K * Ld)[1] == 40
    with pytest.raises(ValueError, match="^criterion must be 'bic' or 'aic', got 'icl'$"):
        _select((2, 3), {2: 0.0, 3: 0.0}, "icl")
    with pytest.raises(ValueError, match="^ks is empty$"):
        _select((), {})


class _Fit:
    """a state {done, n_iter, why, 0} on the host; iteration done_at sets done, as the decide kernels do, and every
    step behind the decision returns at once"""

    def __init__(self, done_at=None):
        self.state = torch.zeros(4, dtype=torch.int32)
        self.done_at, self.calls = done_at, []

    def step(self, it):
        self.calls.append(it)
        if int(self.state[0]):
            return
        self.state[1] += 1
        if self.done_at is not None and int(self.state[1]) == self.done_at:
            self.state[0], self.state[2] = 1, 7


def test_run_until_done():
    f = _Fit(done_at=11)
    assert H.ENQUEUE == 8 and H.run_until_done(f.step, f.state, 300) == (11, 7, False)
    assert f.calls == list(range(16))                       # two batches of the default 8; the last five returned at once
    f = _Fit(done_at=11)
    assert H.run_until_done(f.step, f.state, 300, enqueue=3) == (11, 7, False) and f.calls == list(range(12))
    f = _Fit(done_at=11)
    assert H.run_until_done(f.step, f.state, 11) == (11, 7, False) and f.calls == list(range(11))
    f = _Fit()                                              # done never sets: never beyond max_iter
    assert H.run_until_done(f.step, f.state, 5) == (5, 0, False) and f.calls == list(range(5))
    f = _Fit()
    assert H.run_until_done(f.step, f.state, 20) == (20, 0, False) and f.calls == list(range(20))


def test_run_until_done_also_stop():
    f = _Fit(done_at=30)
    asked = []

    def also_stop():                                        # turns true during the second batch
        asked.append(len(f.calls))
        return len(f.calls) >= 12

    assert H.run_until_done(f.step, f.state, 300, also_stop=also_stop) == (16, 0, True)
    assert f.calls == list(range(16)) and asked == [8, 16]  # asked once per batch, after the state was read
    f = _Fit(done_at=3)                                     # it goes ahead of done
    assert H.run_until_done(f.step, f.state, 300, also_stop=lambda: True) == (3, 7, True)
    f = _Fit(done_at=3)
    assert H.run_until_done(f.step, f.state, 300, also_stop=lambda: False) == (3, 7, False) and len(f.calls) == 8
