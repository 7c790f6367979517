"""Hidden Markov model of the soft latents in time order: which state is each frame in, given its neighbours?  The
mixture's diagonal Gaussian emissions (mixture.py), a K x K transition matrix that says how long states last and which
follows which, fitted by Baum-Welch on the device (csrc/hmm.hip); a state may be visited any number of times, which
segments.segment's K contiguous runs cannot express, and the posterior is smoothed over time, which the mixture's is not.
  hmm                   EM: rbvae_hmm_emit / _forward / _backward / _posterior, then rbvae_gmm_mstep on the posterior and
                        rbvae_gmm_decide on the per-row log-likelihood -- the mixture's stopping rule and order -- enqueued
                        eight iterations at a time
  hmm_forward_backward  the recursions on any log-emissions [N, K]: posterior, expected transition counts, log-likelihood
  hmm_viterbi           the most likely state sequence for any log-emissions
  hmm_score, hmm_predict (Viterbi), hmm_predict_proba     a fit's parameters on any X of the same L, in time order
  hmm_bic, hmm_aic      -2 score N + p log N and -2 score N + 2 p with p = (K - 1) + K (K - 1) + 2 K L free parameters
  hmm_select            one fit per K, the K with the lowest criterion (mixture.choose)
  latent_hmm            the fit at the number of states of the script's data, scored against the states and the flags
The start is a labelling (symbols.kmeans' by default, as mixture.gmm takes it): the emissions are its one-hot posterior's
M-step, A_ij = (n_ij + 1) / (sum_j n_ij + K) from its transition counts and pi = 1 / K.  Full covariances, several
sequences, priors on A, a blocked Viterbi and matrix-core products are not built; Bernoulli emissions for the hard codes are
bernoulli.bhmm, which runs this module's recursions, posterior and Viterbi on them.
There is no host path: a matrix on the CPU raises.  The shapes are rbvae_hmm_ok's.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Union

import numpy as np
import torch

from . import _lib as L
from . import mixture, symbols
from ._latents import ENQUEUE  # noqa: F401  (the batch of run_until_done)
from ._latents import checked_matrix, encode_frames, frame_count, frame_labels, run_until_done

MAX_STATES = 64                                     # rbvae_hmm_ok
NO_ROW = 2 ** 31 - 1                                # status[1] before any normaliser failed


@dataclass
class HMMResult:
    startprob: torch.Tensor             # f64 [K] on the device: pi
    transmat: torch.Tensor              # f64 [K, K]: A, row-stochastic
    means: torch.Tensor                 # f64 [K, L]
    covariances: torch.Tensor           # f64 [K, L]: the variances
    n_iter: int
    converged: bool
    why: str                            # "converged", "max_iter" or "degenerate" (a normaliser was 0 or not finite)
    log_likelihood: float               # the mean per-row log-likelihood of the last iteration's parameters before its M-step
    log_likelihoods: np.ndarray         # f64 [n_iter]: every iteration's
    posterior: torch.Tensor             # f64 [N, K]: the smoothed posterior under the final parameters
    path: torch.Tensor                  # int32 [N]: the Viterbi path under the final parameters
    path_score: float                   # its log-probability
    precisions_cholesky: torch.Tensor   # f64 [K, L]: 1 / sqrt(covariances), as the M-step wrote it


def _checked(X, K, what):
    return checked_matrix(X, what, "rbvae_hmm_ok", f"1 <= L <= 128, 1 <= K <= {MAX_STATES}, max(K, 2) <= N <= 1048576, "
                          f"N K <= 67108864", K=K)


def _f64(a, name, shape, dev):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    if t.dtype != torch.float64 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be float64 {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return t.to(dev).contiguous()


def _block_rows(block_rows):
    R = L.query("rbvae_hmm_block_rows") if block_rows is None else int(block_rows)
    if R < 1:
        raise ValueError(f"block_rows ({R}) must be at least 1")
    return R


def _status(dev):
    return torch.tensor([0, NO_ROW], dtype=torch.int32, device=dev)


class _Buffers:
    """what one E-step writes, for N rows and K states"""

    def __init__(self, N, K, R, dev):
        f = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)     # noqa: E731
        self.N, self.K, self.R = N, K, R
        self.logb, self.rowmax, self.e = f(K, N), f(N), f(N, K)
        self.alpha, self.beta, self.ll = f(N, K), f(N, K), f(N)
        self.gamma, self.xi = f(K, N), f(K, K)
        self.ws_bytes = L.query("rbvae_hmm_ws_bytes", N, K, R)
        self.ws = f(self.ws_bytes // 8)
        self.status = _status(dev)

    def recursions(self, pi, A, state=None):
        N, K = self.N, self.K
        L.call("rbvae_hmm_forward", self.e, self.rowmax, N, K, pi, A, self.R, self.alpha, self.ll, self.status, self.ws,
               self.ws_bytes, state)
        L.call("rbvae_hmm_backward", self.e, N, K, A, self.R, self.beta, self.status, self.ws, self.ws_bytes, state)

    def posterior(self, A, A_new, pi_new, state=None):
        L.call("rbvae_hmm_posterior", self.alpha, self.beta, self.e, self.N, self.K, A, self.gamma, self.xi, A_new, pi_new,
               self.status, self.ws, self.ws_bytes, state)


def _viterbi(logb, N, K, pi, A):
    """logb f64 [K, N] on the device; log pi and log A are taken on the host (log 0 = -inf)"""
    dev = logb.device
    with np.errstate(divide="ignore"):
        lpi = torch.from_numpy(np.log(pi.cpu().numpy())).to(dev)
        lA = torch.from_numpy(np.log(A.cpu().numpy())).to(dev)
    back = torch.empty((N, K), dtype=torch.uint8, device=dev)
    path = torch.empty(N, dtype=torch.int32, device=dev)
    score = torch.empty(1, dtype=torch.float64, device=dev)
    L.call("rbvae_hmm_viterbi", logb, N, K, lpi, lA, back, path, score, None)
    return path, float(score[0])


def _initial_transitions(lab: torch.Tensor, K: int) -> torch.Tensor:
    """A_ij = (n_ij + 1) / (sum_j n_ij + K) from the labelling's transition counts (integers: exact in f64)"""
    n = torch.zeros(K * K, dtype=torch.int64, device=lab.device)
    n.scatter_add_(0, lab[:-1] * K + lab[1:], torch.ones_like(lab[1:]))
    n = n.view(K, K)
    return ((n + 1).double() / (n.sum(dim=1, keepdim=True) + K).double()).contiguous()


def hmm(X: torch.Tensor, n_states: int, init: Union[str, torch.Tensor, np.ndarray] = "kmeans", max_iter: int = 100,
        tol: float = 1e-3, reg_covar: float = 1e-6, seed: int = 42, block_rows: Optional[int] = None) -> HMMResult:
    """Baum-Welch for an f32 device matrix X [N, L] whose rows are one sequence in time order.  init: "kmeans"
    (symbols.kmeans(X, K, seed=seed).labels) or an integer label vector [N] in [0, K).  An iteration takes the emissions,
    the forward and backward recursions and the posterior under the current parameters, then pi, A (rbvae_hmm_posterior),
    the means and variances (rbvae_gmm_mstep on the posterior; its weights are unused) and decides on the device as the
    mixture does: |mean log-likelihood - previous| < tol -> converged; else n_iter = max_iter -> not converged.  Iterations
    are enqueued ENQUEUE at a time, the state and the status are read once per batch, and launches behind the decision
    return at once.  A normaliser that is 0 or not finite ends the fit as "degenerate".  The posterior and the Viterbi path
    come from one more pass with the final parameters."""
    X, N, Ld, K = _checked(X, n_states, "hmm")
    dev = X.device
    max_iter, tol, reg_covar = mixture.fit_arguments(max_iter, tol, reg_covar)
    R = _block_rows(block_rows)
    lab = mixture.start_labels(X, K, init, seed)
    buf = _Buffers(N, K, R, dev)
    buf.gamma.zero_()
    buf.gamma.scatter_(0, lab.view(1, N), 1.0)
    m = mixture.MStep(X, K, reg_covar)                      # its weights and logc are unused
    means, covars, prec = m.means, m.covars, m.prec
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    lb = torch.full((1,), float("-inf"), dtype=torch.float64, device=dev)
    history = torch.zeros(max_iter, dtype=torch.float64, device=dev)
    m.run(buf.gamma)
    A = _initial_transitions(lab, K)
    pi = torch.full((K,), 1.0 / K, dtype=torch.float64, device=dev)

    def iteration(it):
        L.call("rbvae_hmm_emit", X, N, Ld, means, prec, K, buf.logb, buf.rowmax, buf.e, state)
        buf.recursions(pi, A, state)
        buf.posterior(A, A, pi, state)
        m.run(buf.gamma, state)
        L.call("rbvae_gmm_decide", buf.ll, N, tol, max_iter, lb, history, state)

    n_iter, why, degenerate = run_until_done(iteration, state, max_iter, also_stop=lambda: int(buf.status[0]) != 0)
    scratch_A, scratch_pi = torch.empty_like(A), torch.empty_like(pi)
    L.call("rbvae_hmm_emit", X, N, Ld, means, prec, K, buf.logb, buf.rowmax, buf.e, None)
    buf.recursions(pi, A)
    buf.posterior(A, scratch_A, scratch_pi)
    path, score = _viterbi(buf.logb, N, K, pi, A)
    lls = history[:max(n_iter, 1)].cpu().numpy()
    reason = "degenerate" if degenerate else ("converged" if why == 1 else "max_iter")
    return HMMResult(pi, A, means, covars, int(n_iter), reason == "converged", reason, float(lls[-1]), lls, buf.gamma.t(),
                     path, score, prec)


def _log_emissions(log_b, pi, A, what):
    if not isinstance(log_b, torch.Tensor) or not log_b.is_cuda:
        raise ValueError(f"{what}: log_b must be on the GPU (there is no CPU path)")
    if log_b.dim() != 2 or log_b.dtype != torch.float64:
        raise ValueError(f"{what}: log_b must be a 2-D float64 tensor, got {log_b.dtype} {tuple(log_b.shape)}")
    N, K = log_b.shape
    if L.query("rbvae_hmm_ok", N, 1, K) != 1:
        raise ValueError(f"{what}: (N={N}, K={K}) outside 1 <= K <= {MAX_STATES}, max(K, 2) <= N <= 1048576, N K <= 67108864")
    return N, K, _f64(pi, "pi", (K,), log_b.device), _f64(A, "A", (K, K), log_b.device)


def hmm_forward_backward(log_b: torch.Tensor, pi, A, block_rows: Optional[int] = None):
    """The recursions for any log-emissions log_b f64 [N, K] on the device (rows in time order), pi [K] and a row-stochastic
    A [K, K]; the shift by the row maximum and the exp are torch's.
    -> (gamma f64 [N, K], Xi f64 [K, K], the per-row log-likelihood f64 [N], their sum in rbvae_gmm_decide's order)"""
    N, K, pi, A = _log_emissions(log_b, pi, A, "hmm_forward_backward")
    buf = _Buffers(N, K, _block_rows(block_rows), log_b.device)
    buf.rowmax = log_b.max(dim=1).values.contiguous()
    buf.e = torch.exp(log_b - buf.rowmax[:, None]).contiguous()
    buf.recursions(pi, A)
    buf.posterior(A, torch.empty_like(A), torch.empty_like(pi))
    return buf.gamma.t(), buf.xi, buf.ll, mixture._mean_in_order(buf.ll) * N


def hmm_viterbi(log_b: torch.Tensor, pi, A):
    """The most likely state sequence for log-emissions log_b f64 [N, K] on the device -> (path int32 [N], its
    log-probability); a tie goes to the lower state."""
    N, K, pi, A = _log_emissions(log_b, pi, A, "hmm_viterbi")
    return _viterbi(log_b.t().contiguous(), N, K, pi, A)


def _estep(fit: HMMResult, X, what, posterior=False):
    K = fit.means.shape[0]
    X, N, Ld, K = _checked(X, K, what)
    if Ld != fit.means.shape[1]:
        raise ValueError(f"{what}: X has {Ld} columns, the fit {fit.means.shape[1]}")
    buf = _Buffers(N, K, _block_rows(None), X.device)
    L.call("rbvae_hmm_emit", X, N, Ld, fit.means, fit.precisions_cholesky, K, buf.logb, buf.rowmax, buf.e, None)
    if posterior is not None:
        buf.recursions(fit.startprob, fit.transmat)
    if posterior:
        buf.posterior(fit.transmat, torch.empty_like(fit.transmat), torch.empty_like(fit.startprob))
    return buf


def hmm_score_samples(fit: HMMResult, X: torch.Tensor) -> torch.Tensor:
    """f64 [N] on the device: ll_t = log p(x_t | x_0 .. x_(t-1)); their sum is the sequence's log-likelihood"""
    return _estep(fit, X, "hmm_score_samples").ll


def hmm_score(fit: HMMResult, X: torch.Tensor) -> float:
    """the mean per-row log-likelihood of the sequence X, added on the device in rbvae_gmm_decide's order (gmm_score's
    footing)"""
    return mixture._mean_in_order(hmm_score_samples(fit, X))


def hmm_predict(fit: HMMResult, X: torch.Tensor) -> torch.Tensor:
    """int32 [N] on the device: the Viterbi path of the sequence X"""
    buf = _estep(fit, X, "hmm_predict", posterior=None)
    return _viterbi(buf.logb, buf.N, buf.K, fit.startprob, fit.transmat)[0]


def hmm_predict_proba(fit: HMMResult, X: torch.Tensor) -> torch.Tensor:
    """f64 [N, K] on the device: the smoothed posterior of the sequence X"""
    return _estep(fit, X, "hmm_predict_proba", posterior=True).gamma.t()


def n_parameters(K: int, Ld: int) -> int:
    """K - 1 start probabilities, K (K - 1) transition probabilities, K L means and K L variances"""
    return (K - 1) + K * (K - 1) + 2 * K * Ld


def _criteria(score: float, N: int, K: int, Ld: int):
    return mixture.criteria(score, N, n_parameters(K, Ld))


def hmm_bic(fit: HMMResult, X: torch.Tensor) -> float:
    """-2 score(X) N + p log N"""
    return _criteria(hmm_score(fit, X), X.shape[0], *fit.means.shape)[0]


def hmm_aic(fit: HMMResult, X: torch.Tensor) -> float:
    """-2 score(X) N + 2 p"""
    return _criteria(hmm_score(fit, X), X.shape[0], *fit.means.shape)[1]


def hmm_select(X: torch.Tensor, ks: Sequence[int], criterion: str = "bic", seed: int = 42, **fit_kwargs):
    """mixture.select with hmm, hmm_score and n_parameters -> (table: a list of {"K", "n_iter", "converged", "score", "bic",
    "aic"} in ks' order, the chosen K (mixture.choose: the lowest criterion, a tie to the smaller K), its HMMResult)"""
    return mixture.select(X, ks, criterion, lambda K: hmm(X, K, seed=seed, **fit_kwargs), lambda fit: hmm_score(fit, X),
                          n_parameters)


def change_points(path) -> list:
    """the positions t >= 1 at which path[t] differs from path[t - 1], ascending"""
    p = path.cpu().numpy() if isinstance(path, torch.Tensor) else np.asarray(path)
    return [int(t) for t in np.flatnonzero(p[1:] != p[:-1]) + 1]


@torch.no_grad()
def latent_hmm(model, x: torch.Tensor, frame_indices: Sequence[int], flags: Sequence[int], n_states: Optional[int] = None,
               tolerance: int = 2, projections: Optional[dict] = None, temperature: float = 0.2, noise_ratio: float = 0.3,
               u=None, max_iter: int = 100, tol: float = 1e-3, reg_covar: float = 1e-6, seed: int = 42) -> dict:
    """The model of the script's data in one call: x [F, C, H, W] frames (or latents) on the device in time order, encoded
    by _latents.encode_frames' soft pass (projections["latents"] is used instead when present); the states are
    data.assign_label(frame_indices[f], flags) and n_states defaults to their number, len(flags) + 1.
    -> {"latents", "labels" (the states), "hmm": HMMResult, "agreement": clustering_agreement of the Viterbi path against the
        states, "kmeans_agreement": the same for the k-means start, "change_points", "boundaries": segments.boundary_agreement
        of the change points against the positions where the state changes, at `tolerance`, "dwell": f64 [K] on the host,
        1 / (1 - A_kk), "mean_max_posterior"}"""
    from .segments import boundary_agreement
    labels = frame_labels(frame_indices, flags, frame_count(x))
    S = len(flags) + 1
    K = S if n_states is None else int(n_states)
    z, _ = encode_frames(model, x, hard=False, latents=projections.get("latents") if projections is not None else None,
                         temperature=temperature, noise_ratio=noise_ratio, u=u)
    start = symbols.kmeans(z, K, seed=seed).labels
    fit = hmm(z, K, init=start, max_iter=max_iter, tol=tol, reg_covar=reg_covar, seed=seed)
    cps = change_points(fit.path)
    with np.errstate(divide="ignore"):
        dwell = 1.0 / (1.0 - torch.diagonal(fit.transmat).cpu().numpy())
    return {"latents": z, "labels": labels, "hmm": fit, "agreement": symbols.clustering_agreement(labels, fit.path, S, K),
            "kmeans_agreement": symbols.clustering_agreement(labels, start, S, K), "change_points": cps,
            "boundaries": boundary_agreement(cps, change_points(labels), tolerance), "dwell": dwell,
            "mean_max_posterior": float(fit.posterior.max(dim=1).values.mean())}
