"""Gaussian mixture of the soft latents: how many states are there, and how sure is each frame's?  A diagonal-covariance
mixture fitted by EM on the device (csrc/gmm.hip) as scikit-learn 1.7.2's GaussianMixture(covariance_type="diag", n_init=1,
init_params="kmeans") fits it.  Its likelihood gives BIC and AIC, so a number of states is chosen without the flags; its
responsibilities are soft symbols; its per-frame log-likelihood drops where a frame fits no state.
  gmm                   EM (rbvae_gmm_estep / _mstep / _decide), enqueued eight iterations at a time: the decision is taken
                        on the device after every iteration and later launches return at once
  gmm_predict_proba, gmm_predict, gmm_score_samples, gmm_score      one E-step with a fit's parameters on any X of the same L
  gmm_bic, gmm_aic      -2 score N + p log N and -2 score N + 2 p with p = 2 K L + K - 1 free parameters
  gmm_select            one fit per K, the K with the lowest criterion (ties to the smaller K)
  latent_mixture        the fit at the number of states for the script's data, scored against the states
  fit_arguments, start_labels, MStep, criteria, select      what hmm.py's Baum-Welch shares with this fit
The start is symbols.kmeans' labelling (scikit-learn's own start: KMeans(n_clusters=K, n_init=1) from the same RandomState)
or any labelling; its one-hot responsibilities go through one M-step (which divides the weights by their sum, where
scikit-learn's initialisation divides by N: the sums differ by K * 10 * 2^-52).  Full, tied and spherical covariance,
n_init > 1, the other init_params and warm start are not built; the Bernoulli mixture for the hard codes is bernoulli.bmm.
There is no host path: a matrix on the CPU raises.  The shapes are rbvae_gmm_ok's, also for prediction: X needs at least K rows.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Union

import numpy as np
import torch

from . import _lib as L
from . import symbols
from ._latents import ENQUEUE  # noqa: F401  (the batch of run_until_done)
from ._latents import checked_matrix, encode_frames, frame_count, frame_labels, run_until_done

MAX_COMPONENTS = 256                                # rbvae_gmm_ok


@dataclass
class GMMResult:
    weights: torch.Tensor               # f64 [K] on the device
    means: torch.Tensor                 # f64 [K, L]
    covariances: torch.Tensor           # f64 [K, L]: the variances
    n_iter: int
    converged: bool
    lower_bound: float                  # the mean log-likelihood of the last iteration's E-step (scikit-learn's lower_bound_)
    lower_bounds: np.ndarray            # f64 [n_iter]: every iteration's
    labels: torch.Tensor                # int32 [N]: the most likely component under the final parameters (fit_predict)
    precisions_cholesky: torch.Tensor   # f64 [K, L]: 1 / sqrt(covariances), as the M-step wrote it
    log_const: torch.Tensor             # f64 [K]: log w_k + sum_l log s_kl - L / 2 log 2 pi, as the M-step wrote it


def _checked(X, K, what):
    return checked_matrix(X, what, "rbvae_gmm_ok", f"1 <= L <= 128, 1 <= K <= {MAX_COMPONENTS}, K <= N <= 1048576, "
                          f"N K <= 67108864", K=K)


def _mean_in_order(v: torch.Tensor) -> float:
    """the mean of an f64 device vector in rbvae_gmm_decide's fixed order"""
    dev = v.device
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    lb = torch.full((1,), float("-inf"), dtype=torch.float64, device=dev)
    hist = torch.empty(1, dtype=torch.float64, device=dev)
    L.call("rbvae_gmm_decide", v, v.shape[0], 0.0, 1, lb, hist, state)
    return float(hist[0])


def fit_arguments(max_iter, tol, reg_covar):
    """-> (max_iter, tol, reg_covar) as int, float, float; what gmm and hmm.hmm refuse, they refuse in these words"""
    max_iter = int(max_iter)
    if max_iter < 1 or not tol >= 0 or not reg_covar >= 0:
        raise ValueError(f"max_iter ({max_iter}) must be at least 1, tol ({tol}) and reg_covar ({reg_covar}) non-negative")
    return max_iter, float(tol), float(reg_covar)


def start_labels(X, K, init, seed) -> torch.Tensor:
    """the labelling a fit starts from -> int64 [N] on X's device: symbols.kmeans' for init "kmeans", else init itself"""
    N = X.shape[0]
    if isinstance(init, str):
        if init != "kmeans":
            raise ValueError(f"init must be 'kmeans' or a label vector, got {init!r}")
        return symbols.kmeans(X, K, seed=seed).labels.long()
    lab = symbols._device_labels(init, "init", X.device)
    if lab.shape[0] != N or int(lab.min()) < 0 or int(lab.max()) >= K:
        raise ValueError(f"init must be {N} labels in [0, {K}), got {tuple(lab.shape)}")
    return lab


class MStep:
    """rbvae_gmm_mstep's outputs and workspace for X [N, L] and K components; run(resp, state) fills them from resp [K, N]"""

    def __init__(self, X, K, reg_covar):
        N, Ld = X.shape
        f = lambda *s: torch.empty(s, dtype=torch.float64, device=X.device)     # noqa: E731
        self.X, self.K, self.reg_covar = X, K, reg_covar
        self.weights, self.logc, self.means, self.covars, self.prec = f(K), f(K), f(K, Ld), f(K, Ld), f(K, Ld)
        self.ws = f(L.query("rbvae_gmm_ws_bytes", N, Ld, K) // 8)

    def run(self, resp, state=None):
        N, Ld = self.X.shape
        L.call("rbvae_gmm_mstep", self.X, N, Ld, resp, self.K, self.reg_covar, self.weights, self.means, self.covars,
               self.prec, self.logc, self.ws, state)


def gmm(X: torch.Tensor, n_components: int, init: Union[str, torch.Tensor, np.ndarray] = "kmeans", max_iter: int = 100,
        tol: float = 1e-3, reg_covar: float = 1e-6, seed: int = 42) -> GMMResult:
    """GaussianMixture(n_components, covariance_type="diag", n_init=1, init_params="kmeans", max_iter=max_iter, tol=tol,
    reg_covar=reg_covar, random_state=seed).fit(X) for an f32 device matrix X [N, L].  init: "kmeans"
    (symbols.kmeans(X, K, seed=seed).labels) or an integer label vector [N] in [0, K).  An iteration takes the
    responsibilities under the current parameters (E), the parameters from them (M) and then decides on the device:
    |lower bound - previous| < tol -> converged; else n_iter = max_iter -> not converged.  Iterations are enqueued ENQUEUE
    at a time and the state is read once per batch; launches behind the decision return at once, so the result is that of
    a check after every iteration.  The labels come from one more E-step with the final parameters."""
    X, N, Ld, K = _checked(X, n_components, "gmm")
    dev = X.device
    max_iter, tol, reg_covar = fit_arguments(max_iter, tol, reg_covar)
    lab = start_labels(X, K, init, seed)
    resp = torch.zeros((K, N), dtype=torch.float64, device=dev)
    resp.scatter_(0, lab.view(1, N), 1.0)
    m = MStep(X, K, reg_covar)
    lognorm = torch.empty(N, dtype=torch.float64, device=dev)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    lb = torch.full((1,), float("-inf"), dtype=torch.float64, device=dev)
    history = torch.zeros(max_iter, dtype=torch.float64, device=dev)
    m.run(resp)

    def iteration(it):
        L.call("rbvae_gmm_estep", X, N, Ld, m.means, m.prec, m.logc, K, resp, lognorm, None, state)
        m.run(resp, state)
        L.call("rbvae_gmm_decide", lognorm, N, tol, max_iter, lb, history, state)

    n_iter, why, _ = run_until_done(iteration, state, max_iter)
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    L.call("rbvae_gmm_estep", X, N, Ld, m.means, m.prec, m.logc, K, None, lognorm, labels, None)
    bounds = history[:n_iter].cpu().numpy()
    return GMMResult(m.weights, m.means, m.covars, int(n_iter), why == 1, float(bounds[-1]), bounds, labels, m.prec, m.logc)


def _estep(fit: GMMResult, X, what, want_resp=False, want_label=False):
    K = fit.means.shape[0]
    X, N, Ld, K = _checked(X, K, what)
    if Ld != fit.means.shape[1]:
        raise ValueError(f"{what}: X has {Ld} columns, the fit {fit.means.shape[1]}")
    dev = X.device
    resp = torch.empty((K, N), dtype=torch.float64, device=dev) if want_resp else None
    label = torch.empty(N, dtype=torch.int32, device=dev) if want_label else None
    lognorm = torch.empty(N, dtype=torch.float64, device=dev)
    L.call("rbvae_gmm_estep", X, N, Ld, fit.means, fit.precisions_cholesky, fit.log_const, K, resp, lognorm, label, None)
    return resp, lognorm, label


def gmm_predict_proba(fit: GMMResult, X: torch.Tensor) -> torch.Tensor:
    """predict_proba(X) -> f64 [N, K] on the device (a view of the kernel's component-major [K, N])"""
    return _estep(fit, X, "gmm_predict_proba", want_resp=True)[0].t()


def gmm_predict(fit: GMMResult, X: torch.Tensor) -> torch.Tensor:
    """predict(X) -> int32 [N] on the device: the component with the largest weighted log-probability, ties to the lower"""
    return _estep(fit, X, "gmm_predict", want_label=True)[2]


def gmm_score_samples(fit: GMMResult, X: torch.Tensor) -> torch.Tensor:
    """score_samples(X) -> f64 [N] on the device: each row's log-likelihood under the mixture"""
    return _estep(fit, X, "gmm_score_samples")[1]


def gmm_score(fit: GMMResult, X: torch.Tensor) -> float:
    """score(X): the mean of score_samples, added on the device in rbvae_gmm_decide's order"""
    return _mean_in_order(gmm_score_samples(fit, X))


def n_parameters(K: int, Ld: int) -> int:
    """the free parameters of a diagonal mixture: K L means, K L variances and K - 1 weights"""
    return 2 * K * Ld + K - 1


def criteria(score: float, N: int, p: int):
    """(BIC, AIC) = (-2 score N + p log N, -2 score N + 2 p) of a mean log-likelihood over N rows with p free parameters"""
    return -2.0 * score * N + p * math.log(N), -2.0 * score * N + 2.0 * p


def gmm_bic(fit: GMMResult, X: torch.Tensor) -> float:
    """bic(X) = -2 score(X) N + p log N"""
    return criteria(gmm_score(fit, X), X.shape[0], n_parameters(*fit.means.shape))[0]


def gmm_aic(fit: GMMResult, X: torch.Tensor) -> float:
    """aic(X) = -2 score(X) N + 2 p"""
    return criteria(gmm_score(fit, X), X.shape[0], n_parameters(*fit.means.shape))[1]


def choose(table, criterion="bic") -> int:
    """the row of the table with the lowest criterion; a tie goes to the smaller K"""
    if criterion not in ("bic", "aic"):
        raise ValueError(f"criterion must be 'bic' or 'aic', got {criterion!r}")
    return min(range(len(table)), key=lambda j: (table[j][criterion], table[j]["K"]))


def select(X, ks: Sequence[int], criterion: str, fit, score, n_parameters):
    """One fit(K) per K in ks, scored by score(fit(K)) -> (table: a list of {"K", "n_iter", "converged", "score", "bic",
    "aic"} in ks' order, the chosen K (choose: the lowest criterion, a tie to the smaller K), its fit).  The criteria are
    those of X's N rows and n_parameters(K, L) free parameters; fit is what checks X."""
    ks = [int(k) for k in ks]
    if not ks:
        raise ValueError("ks is empty")
    if criterion not in ("bic", "aic"):
        raise ValueError(f"criterion must be 'bic' or 'aic', got {criterion!r}")
    table, fits = [], []
    for K in ks:
        f = fit(K)
        s = score(f)
        bic, aic = criteria(s, X.shape[0], n_parameters(K, X.shape[1]))
        table.append({"K": K, "n_iter": f.n_iter, "converged": f.converged, "score": s, "bic": bic, "aic": aic})
        fits.append(f)
    j = choose(table, criterion)
    return table, ks[j], fits[j]


def gmm_select(X: torch.Tensor, ks: Sequence[int], criterion: str = "bic", seed: int = 42, **fit_kwargs):
    """One fit per K in ks (select with gmm, gmm_score and n_parameters) -> (table: a list of {"K", "n_iter", "converged",
    "score", "bic", "aic"} in ks' order, the chosen K, its GMMResult).  score is the mean log-likelihood under the final
    parameters, not lower_bound."""
    return select(X, ks, criterion, lambda K: gmm(X, K, seed=seed, **fit_kwargs), lambda fit: gmm_score(fit, X), n_parameters)


@torch.no_grad()
def latent_mixture(model, x: torch.Tensor, frame_indices: Sequence[int], flags: Sequence[int],
                   n_components: Optional[int] = None, ks: Optional[Sequence[int]] = None, criterion: str = "bic",
                   projections: Optional[dict] = None, temperature: float = 0.2, noise_ratio: float = 0.3, u=None,
                   max_iter: int = 100, tol: float = 1e-3, reg_covar: float = 1e-6, seed: int = 42) -> dict:
    """The mixture of the script's data in one call: x [F, C, H, W] frames (or latents) on the device, encoded by
    _latents.encode_frames' soft pass (the uniforms u [F, L]; projections["latents"] is used instead when present); the
    states are data.assign_label(frame_indices[f], flags) and n_components defaults to their number, len(flags) + 1.
    -> {"latents", "labels" (the states), "gmm": GMMResult, "agreement": clustering_agreement of the fit's labels against
        the states, "responsibilities" f64 [F, K], "mean_max_responsibility", "log_likelihood" f64 [F] (gmm_score_samples),
        "entropy" f64 [F] (-sum_k r log r in nats, 0 log 0 = 0), and with ks given "selection": gmm_select's
        (table, chosen K, fit)}"""
    labels = frame_labels(frame_indices, flags, frame_count(x))
    S = len(flags) + 1
    K = S if n_components is None else int(n_components)
    z, _ = encode_frames(model, x, hard=False, latents=projections.get("latents") if projections is not None else None,
                         temperature=temperature, noise_ratio=noise_ratio, u=u)
    kw = dict(max_iter=max_iter, tol=tol, reg_covar=reg_covar)
    fit = gmm(z, K, seed=seed, **kw)
    resp = gmm_predict_proba(fit, z)
    out = {"latents": z, "labels": labels, "gmm": fit, "agreement": symbols.clustering_agreement(labels, fit.labels, S, K),
           "responsibilities": resp, "mean_max_responsibility": float(resp.max(dim=1).values.mean()),
           "log_likelihood": gmm_score_samples(fit, z), "entropy": torch.special.entr(resp).sum(dim=1)}
    if ks is not None:
        out["selection"] = gmm_select(z, ks, criterion=criterion, seed=seed, **kw)
    return out
