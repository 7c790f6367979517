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
  hmm_sequence_scores   the log-likelihood of each of several sequences: which recording does the model explain worst?
  latent_hmm_videos     one model of several videos (or of all but one, which is then labelled from the others)
Several sequences: every function that takes a sequence takes lengths=(n_0, n_1, ...), the rows of the sequences stacked in
time order (sum = N).  The recursions, the posterior and Viterbi then run per sequence (the rbvae_hmm_seq_ entries and their
device plan, built once per call): no transition is counted or smoothed across a boundary, every sequence starts from pi, and
pi is the mean of the sequences' first posteriors.  lengths=None makes exactly the single-sequence calls.
The start is a labelling (symbols.kmeans' by default, as mixture.gmm takes it): the emissions are its one-hot posterior's
M-step, A_ij = (n_ij + 1) / (sum_j n_ij + K) from its transition counts (within the sequences) and pi = 1 / K.  Full
covariances, per-sequence weights, priors on A, a blocked Viterbi and matrix-core products are not built; Bernoulli emissions
for the hard codes are bernoulli.bhmm, which runs this module's recursions, posterior and Viterbi on them.
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
    lengths: Optional[tuple] = None     # the lengths of the sequences the fit saw (None: one sequence)
    path_scores: Optional[np.ndarray] = None    # f64 [S]: every sequence's path log-probability; path_score is their sum


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


def _lengths(lengths, N, what):
    """None, or the lengths as a tuple of ints: every one at least 1, their sum N"""
    if lengths is None:
        return None
    ls = tuple(int(n) for n in lengths)
    if not ls or min(ls) < 1 or sum(ls) != N:
        raise ValueError(f"{what}: lengths must be positive and add to the {N} rows, got {len(ls)} lengths that add to {sum(ls)}"
                         + (f" (the smallest is {min(ls)})" if ls else ""))
    return ls


class _Plan:
    """the device plan of several stacked sequences (rbvae_hmm_seq_plan): built once, used by every entry of a call"""

    def __init__(self, lengths, N, R, dev):
        self.lengths, self.S = lengths, len(lengths)
        nbytes = L.query("rbvae_hmm_seq_plan_bytes", N, self.S, R)
        self.dev = torch.empty(max(nbytes, 4) // 4, dtype=torch.int32, device=dev)
        host = np.ascontiguousarray(lengths, dtype=np.int32)
        L.call("rbvae_hmm_seq_plan", host.ctypes.data, self.S, N, R, self.dev, nbytes)
        self.first = np.concatenate([[0], np.cumsum(host, dtype=np.int64)])        # [S + 1]: every sequence's first row, and N


def _plan(lengths, N, R, dev, what):
    ls = _lengths(lengths, N, what)
    return None if ls is None else _Plan(ls, N, R, dev)


class _Buffers:
    """what one E-step writes, for N rows and K states; plan: the rows are several sequences"""

    def __init__(self, N, K, R, dev, plan=None):
        f = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)     # noqa: E731
        self.N, self.K, self.R, self.plan = N, K, R, plan
        self.logb, self.rowmax, self.e = f(K, N), f(N), f(N, K)
        self.alpha, self.beta, self.ll = f(N, K), f(N, K), f(N)
        self.gamma, self.xi = f(K, N), f(K, K)
        self.ws_bytes = (L.query("rbvae_hmm_ws_bytes", N, K, R) if plan is None
                         else L.query("rbvae_hmm_seq_ws_bytes", N, K, plan.S, R))
        self.ws = f(self.ws_bytes // 8)
        self.status = _status(dev)

    def recursions(self, pi, A, state=None):
        N, K, p = self.N, self.K, self.plan
        if p is None:
            L.call("rbvae_hmm_forward", self.e, self.rowmax, N, K, pi, A, self.R, self.alpha, self.ll, self.status, self.ws,
                   self.ws_bytes, state)
            L.call("rbvae_hmm_backward", self.e, N, K, A, self.R, self.beta, self.status, self.ws, self.ws_bytes, state)
            return
        L.call("rbvae_hmm_seq_forward", self.e, self.rowmax, N, K, pi, A, self.R, p.dev, p.S, self.alpha, self.ll, self.status,
               self.ws, self.ws_bytes, state)
        L.call("rbvae_hmm_seq_backward", self.e, N, K, A, self.R, p.dev, p.S, self.beta, self.status, self.ws, self.ws_bytes,
               state)

    def posterior(self, A, A_new, pi_new, state=None):
        if self.plan is None:
            L.call("rbvae_hmm_posterior", self.alpha, self.beta, self.e, self.N, self.K, A, self.gamma, self.xi, A_new, pi_new,
                   self.status, self.ws, self.ws_bytes, state)
            return
        L.call("rbvae_hmm_seq_posterior", self.alpha, self.beta, self.e, self.N, self.K, self.plan.dev, self.plan.S, A,
               self.gamma, self.xi, A_new, pi_new, self.status, self.ws, self.ws_bytes, state)


def _viterbi(logb, N, K, pi, A, plan=None):
    """logb f64 [K, N] on the device; log pi and log A are taken on the host (log 0 = -inf) -> (path, its log-probability);
    plan: per sequence, and also the sequences' log-probabilities f64 [S] on the host, whose sum (s ascending) is the second"""
    dev = logb.device
    with np.errstate(divide="ignore"):
        lpi = torch.from_numpy(np.log(pi.cpu().numpy())).to(dev)
        lA = torch.from_numpy(np.log(A.cpu().numpy())).to(dev)
    back = torch.empty((N, K), dtype=torch.uint8, device=dev)
    path = torch.empty(N, dtype=torch.int32, device=dev)
    if plan is None:
        score = torch.empty(1, dtype=torch.float64, device=dev)
        L.call("rbvae_hmm_viterbi", logb, N, K, lpi, lA, back, path, score, None)
        return path, float(score[0])
    scores = torch.empty(plan.S, dtype=torch.float64, device=dev)
    L.call("rbvae_hmm_seq_viterbi", logb, N, K, plan.dev, plan.S, lpi, lA, back, path, scores, None)
    scores = scores.cpu().numpy()
    return path, _sum_ascending(scores), scores


def _sum_ascending(a) -> float:
    """one running sum from zero, in index order"""
    return float(np.cumsum(np.asarray(a, dtype=np.float64))[-1])


def _initial_transitions(lab: torch.Tensor, K: int, plan=None) -> torch.Tensor:
    """A_ij = (n_ij + 1) / (sum_j n_ij + K) from the labelling's transition counts (integers: exact in f64); plan: a pair
    across a boundary of two sequences is not a transition"""
    n = torch.zeros(K * K, dtype=torch.int64, device=lab.device)
    ones = torch.ones_like(lab[1:])
    if plan is not None:
        ones[torch.from_numpy(plan.first[1:-1] - 1).to(lab.device)] = 0
    n.scatter_add_(0, lab[:-1] * K + lab[1:], ones)
    n = n.view(K, K)
    return ((n + 1).double() / (n.sum(dim=1, keepdim=True) + K).double()).contiguous()


def hmm(X: torch.Tensor, n_states: int, init: Union[str, torch.Tensor, np.ndarray] = "kmeans", max_iter: int = 100,
        tol: float = 1e-3, reg_covar: float = 1e-6, seed: int = 42, block_rows: Optional[int] = None,
        lengths: Optional[Sequence[int]] = None) -> HMMResult:
    """Baum-Welch for an f32 device matrix X [N, L] whose rows are one sequence in time order, or with lengths several,
    stacked (k-means, the M-step on the pooled posterior and the decision on all N rows do not ask).  init: "kmeans"
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
    plan = _plan(lengths, N, R, dev, "hmm")
    buf = _Buffers(N, K, R, dev, plan)
    buf.gamma.zero_()
    buf.gamma.scatter_(0, lab.view(1, N), 1.0)
    m = mixture.MStep(X, K, reg_covar)                      # its weights and logc are unused
    means, covars, prec = m.means, m.covars, m.prec
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    lb = torch.full((1,), float("-inf"), dtype=torch.float64, device=dev)
    history = torch.zeros(max_iter, dtype=torch.float64, device=dev)
    m.run(buf.gamma)
    A = _initial_transitions(lab, K, plan)
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
    path, score, *scores = _viterbi(buf.logb, N, K, pi, A, plan)
    lls = history[:max(n_iter, 1)].cpu().numpy()
    reason = "degenerate" if degenerate else ("converged" if why == 1 else "max_iter")
    return HMMResult(pi, A, means, covars, int(n_iter), reason == "converged", reason, float(lls[-1]), lls, buf.gamma.t(),
                     path, score, prec, *((plan.lengths, scores[0]) if plan is not None else ()))


def _log_emissions(log_b, pi, A, what):
    if not isinstance(log_b, torch.Tensor) or not log_b.is_cuda:
        raise ValueError(f"{what}: log_b must be on the GPU (there is no CPU path)")
    if log_b.dim() != 2 or log_b.dtype != torch.float64:
        raise ValueError(f"{what}: log_b must be a 2-D float64 tensor, got {log_b.dtype} {tuple(log_b.shape)}")
    N, K = log_b.shape
    if L.query("rbvae_hmm_ok", N, 1, K) != 1:
        raise ValueError(f"{what}: (N={N}, K={K}) outside 1 <= K <= {MAX_STATES}, max(K, 2) <= N <= 1048576, N K <= 67108864")
    return N, K, _f64(pi, "pi", (K,), log_b.device), _f64(A, "A", (K, K), log_b.device)


def hmm_forward_backward(log_b: torch.Tensor, pi, A, block_rows: Optional[int] = None,
                         lengths: Optional[Sequence[int]] = None):
    """The recursions for any log-emissions log_b f64 [N, K] on the device (rows in time order; with lengths several
    sequences, stacked), pi [K] and a row-stochastic A [K, K]; the shift by the row maximum and the exp are torch's.
    -> (gamma f64 [N, K], Xi f64 [K, K], the per-row log-likelihood f64 [N], their sum in rbvae_gmm_decide's order)"""
    N, K, pi, A = _log_emissions(log_b, pi, A, "hmm_forward_backward")
    R = _block_rows(block_rows)
    buf = _Buffers(N, K, R, log_b.device, _plan(lengths, N, R, log_b.device, "hmm_forward_backward"))
    buf.rowmax = log_b.max(dim=1).values.contiguous()
    buf.e = torch.exp(log_b - buf.rowmax[:, None]).contiguous()
    buf.recursions(pi, A)
    buf.posterior(A, torch.empty_like(A), torch.empty_like(pi))
    return buf.gamma.t(), buf.xi, buf.ll, mixture._mean_in_order(buf.ll) * N


def hmm_viterbi(log_b: torch.Tensor, pi, A, lengths: Optional[Sequence[int]] = None):
    """The most likely state sequence for log-emissions log_b f64 [N, K] on the device -> (path int32 [N], its
    log-probability); a tie goes to the lower state.  With lengths every sequence has its own path:
    -> (path, the sum of their log-probabilities, those log-probabilities f64 [S] on the host)."""
    N, K, pi, A = _log_emissions(log_b, pi, A, "hmm_viterbi")
    return _viterbi(log_b.t().contiguous(), N, K, pi, A, _plan(lengths, N, _block_rows(None), log_b.device, "hmm_viterbi"))


def _estep(fit: HMMResult, X, what, posterior=False, lengths=None):
    K = fit.means.shape[0]
    X, N, Ld, K = _checked(X, K, what)
    if Ld != fit.means.shape[1]:
        raise ValueError(f"{what}: X has {Ld} columns, the fit {fit.means.shape[1]}")
    R = _block_rows(None)
    buf = _Buffers(N, K, R, X.device, _plan(lengths, N, R, X.device, what))
    L.call("rbvae_hmm_emit", X, N, Ld, fit.means, fit.precisions_cholesky, K, buf.logb, buf.rowmax, buf.e, None)
    if posterior is not None:
        buf.recursions(fit.startprob, fit.transmat)
    if posterior:
        buf.posterior(fit.transmat, torch.empty_like(fit.transmat), torch.empty_like(fit.startprob))
    return buf


def hmm_score_samples(fit: HMMResult, X: torch.Tensor, lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
    """f64 [N] on the device: ll_t = log p(x_t | x_0 .. x_(t-1)), the earlier rows of its own sequence; a sequence's sum is its
    log-likelihood"""
    return _estep(fit, X, "hmm_score_samples", lengths=lengths).ll


def hmm_score(fit: HMMResult, X: torch.Tensor, lengths: Optional[Sequence[int]] = None) -> float:
    """the mean per-row log-likelihood of the sequence (or sequences) X, added on the device in rbvae_gmm_decide's order
    (gmm_score's footing)"""
    return mixture._mean_in_order(hmm_score_samples(fit, X, lengths))


def hmm_sequence_scores(fit: HMMResult, X: torch.Tensor, lengths: Sequence[int]) -> np.ndarray:
    """f64 [S] on the host: every sequence's log-likelihood, the sum of its ll_t with t ascending -- which recording does the
    model explain worst?"""
    ll = hmm_score_samples(fit, X, lengths).cpu().numpy()
    first = np.concatenate([[0], np.cumsum(_lengths(lengths, len(ll), "hmm_sequence_scores"))])
    return np.array([_sum_ascending(ll[a:b]) for a, b in zip(first[:-1], first[1:])], dtype=np.float64)


def hmm_predict(fit: HMMResult, X: torch.Tensor, lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
    """int32 [N] on the device: the Viterbi path of the sequence X (of every sequence of X)"""
    buf = _estep(fit, X, "hmm_predict", posterior=None, lengths=lengths)
    return _viterbi(buf.logb, buf.N, buf.K, fit.startprob, fit.transmat, buf.plan)[0]


def hmm_predict_proba(fit: HMMResult, X: torch.Tensor, lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
    """f64 [N, K] on the device: the smoothed posterior of the sequence X (of every sequence of X)"""
    return _estep(fit, X, "hmm_predict_proba", posterior=True, lengths=lengths).gamma.t()


def n_parameters(K: int, Ld: int) -> int:
    """K - 1 start probabilities, K (K - 1) transition probabilities, K L means and K L variances"""
    return (K - 1) + K * (K - 1) + 2 * K * Ld


def _criteria(score: float, N: int, K: int, Ld: int):
    return mixture.criteria(score, N, n_parameters(K, Ld))


def hmm_bic(fit: HMMResult, X: torch.Tensor, lengths: Optional[Sequence[int]] = None) -> float:
    """-2 score(X) N + p log N (several sequences have the same parameters)"""
    return _criteria(hmm_score(fit, X, lengths), X.shape[0], *fit.means.shape)[0]


def hmm_aic(fit: HMMResult, X: torch.Tensor, lengths: Optional[Sequence[int]] = None) -> float:
    """-2 score(X) N + 2 p"""
    return _criteria(hmm_score(fit, X, lengths), X.shape[0], *fit.means.shape)[1]


def hmm_select(X: torch.Tensor, ks: Sequence[int], criterion: str = "bic", seed: int = 42,
               lengths: Optional[Sequence[int]] = None, **fit_kwargs):
    """mixture.select with hmm, hmm_score and n_parameters -> (table: a list of {"K", "n_iter", "converged", "score", "bic",
    "aic"} in ks' order, the chosen K (mixture.choose: the lowest criterion, a tie to the smaller K), its HMMResult)"""
    if lengths is not None:
        fit_kwargs["lengths"] = lengths
    return mixture.select(X, ks, criterion, lambda K: hmm(X, K, seed=seed, **fit_kwargs),
                          lambda fit: hmm_score(fit, X, lengths), n_parameters)


def change_points(path, lengths: Optional[Sequence[int]] = None) -> list:
    """the positions t >= 1 at which path[t] differs from path[t - 1], ascending; with lengths the first row of a sequence is
    no change"""
    p = path.cpu().numpy() if isinstance(path, torch.Tensor) else np.asarray(path)
    change = p[1:] != p[:-1]
    ls = _lengths(lengths, len(p), "change_points")
    if ls is not None:
        change[np.cumsum(ls)[:-1] - 1] = False
    return [int(t) for t in np.flatnonzero(change) + 1]


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


@torch.no_grad()
def latent_hmm_videos(model, videos: Sequence[torch.Tensor], frame_indices: Sequence[Sequence[int]],
                      flags: Sequence[Sequence[int]], n_states: Optional[int] = None, holdout: Optional[int] = None,
                      tolerance: int = 2, temperature: float = 0.2, noise_ratio: float = 0.3, u: Optional[Sequence] = None,
                      max_iter: int = 100, tol: float = 1e-3, reg_covar: float = 1e-6, seed: int = 42) -> dict:
    """One model of several videos of the same task: videos[v] [F_v, C, H, W] frames (or latents) on the device, encoded one by
    one as latent_hmm encodes its video (u[v]: the noise of video v), with frame_indices[v] and flags[v] their own; n_states
    defaults to the largest number of states of a video.  The model is fitted on all videos stacked, or on all but
    videos[holdout], which is then labelled with the states learned on the others.
    -> {"latents": [z_v], "labels": [the states of video v], "lengths": of the fitted videos in their order, "hmm": HMMResult,
        "videos": [{"fitted", "path", "agreement": clustering_agreement of its Viterbi path against its own states,
        "change_points", "boundaries": segments.boundary_agreement at `tolerance`}, ...]}: a fitted video's path is its rows of
        hmm.path; the held-out video's is hmm_predict on that video alone (its rows of a prediction on all videos stacked
        would be the same bits), and its entry names the same two scores "predict_agreement" and "predict_boundaries" as
        well, to say where they come from."""
    from .segments import boundary_agreement
    V = len(videos)
    if V < 1 or len(frame_indices) != V or len(flags) != V or (u is not None and len(u) != V):
        raise ValueError(f"latent_hmm_videos: {V} videos need as many frame_indices, flags (and u), got {len(frame_indices)}, "
                         f"{len(flags)}" + (f", {len(u)}" if u is not None else ""))
    if holdout is not None and not (0 <= int(holdout) < V and V >= 2):
        raise ValueError(f"latent_hmm_videos: holdout ({holdout}) must name one of at least two videos")
    labels = [frame_labels(frame_indices[v], flags[v], frame_count(videos[v])) for v in range(V)]
    states = [len(f) + 1 for f in flags]
    K = max(states) if n_states is None else int(n_states)
    z = [encode_frames(model, videos[v], hard=False, temperature=temperature, noise_ratio=noise_ratio,
                       u=None if u is None else u[v])[0] for v in range(V)]
    fitted = [v for v in range(V) if v != holdout]
    lengths = [int(z[v].shape[0]) for v in fitted]
    fit = hmm(torch.cat([z[v] for v in fitted]).contiguous(), K, max_iter=max_iter, tol=tol, reg_covar=reg_covar, seed=seed,
              lengths=lengths)
    paths = dict(zip(fitted, torch.split(fit.path, lengths)))
    if holdout is not None:
        paths[holdout] = hmm_predict(fit, z[holdout])

    def scored(v, path):
        cps = change_points(path)
        return (symbols.clustering_agreement(labels[v], path, states[v], K), cps,
                boundary_agreement(cps, change_points(labels[v]), tolerance))

    out = []
    for v in range(V):
        agreement, cps, bounds = scored(v, paths[v])
        out.append({"fitted": v != holdout, "path": paths[v], "agreement": agreement, "change_points": cps, "boundaries": bounds})
        if v == holdout:
            out[v].update(predict_agreement=agreement, predict_boundaries=bounds)
    return {"latents": z, "labels": labels, "lengths": lengths, "hmm": fit, "videos": out}
