"""Bernoulli models of the hard codes: which state is each frame's code in, when a bit may flip?  A state is a vector of bit
probabilities theta_k, so a frame's likelihood is prod_l theta_kl^x (1 - theta_kl)^(1 - x): the likelihood of 0/1 data, which
the Gaussian mixture.gmm / hmm.hmm are not, and a count of K L + K - 1 parameters for BIC.  Each state gets a prototype code
(theta > 1 / 2) and a per-bit reliability (max(theta, 1 - theta)); the posterior tolerates flipped bits, where
symbols.code_symbols makes every distinct pattern a symbol of its own.  The kernels (csrc/bernoulli.hip) work on bit-packed
codes; the recursions, the posterior, Viterbi and the stop decision are hmm.py's and mixture.py's.
  pack_codes            f32 [N, L] -> int32 [N, 4]: bit l of a row is codes[i, l] > 0.5 (rbvae_bern_pack)
  bmm                   EM of the mixture (rbvae_bern_estep / rbvae_bern_mstep / rbvae_gmm_decide), gmm's loop and stop rule
  bmm_predict_proba, bmm_predict, bmm_score_samples, bmm_score      one E-step with a fit's parameters on any codes of the same L
  bmm_bic, bmm_aic      -2 score N + p log N and -2 score N + 2 p with p = K L + K - 1
  bmm_select            one fit per K, the K with the lowest criterion (mixture.select)
  bhmm                  Baum-Welch with Bernoulli emissions: hmm.hmm's iteration with rbvae_bern_emit for rbvae_hmm_emit and
                        rbvae_bern_mstep for rbvae_gmm_mstep
  bhmm_score_samples, bhmm_score, bhmm_predict (Viterbi), bhmm_predict_proba, bhmm_bic, bhmm_aic, bhmm_select
                        p = (K - 1) + K (K - 1) + K L
  latent_code_models    both fits on the script's data, scored against the states and the flags
The start is a labelling (symbols.kmeans' on the codes by default: Euclidean distance on 0/1 is Hamming distance); its one-hot
responsibilities go through one M-step.  theta_kl = (S_kl + prior) / (nk_k + 2 prior): prior > 0 keeps every log finite.
The bhmm family takes lengths=(n_0, n_1, ...) for several sequences stacked in time order, as hmm.hmm's does (the
rbvae_hmm_seq_ entries).  Priors on A, tied or per-bit-shared probabilities and a categorical model of bit groups are not built.
There is no host path: a matrix on the CPU raises.  The shapes are rbvae_bern_ok's (bhmm: also rbvae_hmm_ok's).
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
from .hmm import MAX_STATES  # noqa: F401  (rbvae_hmm_ok; the package's name hmm is the fit, so the module's names come from .hmm)
from .hmm import _block_rows, _Buffers, _initial_transitions, _plan, _viterbi, change_points

MAX_COMPONENTS = 256                                # rbvae_bern_ok


@dataclass
class BMMResult:
    weights: torch.Tensor               # f64 [K] on the device
    probs: torch.Tensor                 # f64 [K, L]: theta
    log_probs: torch.Tensor             # f64 [K, L]: log theta, as the M-step wrote it
    log_1m_probs: torch.Tensor          # f64 [K, L]: log(1 - theta), as the M-step wrote it
    log_weights: torch.Tensor           # f64 [K]
    n_iter: int
    converged: bool
    lower_bound: float                  # the mean log-likelihood of the last iteration's E-step
    lower_bounds: np.ndarray            # f64 [n_iter]: every iteration's
    labels: torch.Tensor                # int32 [N]: the most likely component under the final parameters


@dataclass
class BHMMResult:
    startprob: torch.Tensor             # f64 [K] on the device: pi
    transmat: torch.Tensor              # f64 [K, K]: A, row-stochastic
    probs: torch.Tensor                 # f64 [K, L]: theta
    log_probs: torch.Tensor             # f64 [K, L]
    log_1m_probs: torch.Tensor          # f64 [K, L]
    n_iter: int
    converged: bool
    why: str                            # "converged", "max_iter" or "degenerate" (a normaliser was 0 or not finite)
    log_likelihood: float               # the mean per-row log-likelihood of the last iteration's parameters before its M-step
    log_likelihoods: np.ndarray         # f64 [n_iter]: every iteration's
    posterior: torch.Tensor             # f64 [N, K]: the smoothed posterior under the final parameters
    path: torch.Tensor                  # int32 [N]: the Viterbi path under the final parameters
    path_score: float                   # its log-probability
    lengths: Optional[tuple] = None     # the lengths of the sequences the fit saw (None: one sequence)
    path_scores: Optional[np.ndarray] = None    # f64 [S]: every sequence's path log-probability; path_score is their sum


def _checked(codes, K, what, chain=False):
    """the codes as a finite f32 device matrix inside rbvae_bern_ok (chain: rbvae_hmm_ok); a shape outside the limits is
    refused before the device is asked for, in checked_matrix's words"""
    ok, limits = (("rbvae_hmm_ok", f"1 <= L <= 128, 1 <= K <= {MAX_STATES}, max(K, 2) <= N <= 1048576, N K <= 67108864") if chain
                  else ("rbvae_bern_ok", f"1 <= L <= 128, 1 <= K <= {MAX_COMPONENTS}, K <= N <= 1048576, N K <= 67108864"))
    if isinstance(codes, torch.Tensor) and codes.dim() == 2 and L.query(ok, codes.shape[0], codes.shape[1], int(K)) != 1:
        raise ValueError(f"{what}: (N={codes.shape[0]}, L={codes.shape[1]}, K={int(K)}) outside {limits}")
    return checked_matrix(codes, what, ok, limits, K=K)


def _arguments(max_iter, tol, prior, init):
    """-> (max_iter, tol, prior); what both fits refuse before they look at the codes"""
    max_iter, tol, _ = mixture.fit_arguments(max_iter, tol, 0.0)
    prior = float(prior)
    if not prior > 0:
        raise ValueError(f"prior ({prior}) must be positive")
    if isinstance(init, str) and init != "kmeans":
        raise ValueError(f"init must be 'kmeans' or a label vector, got {init!r}")
    return max_iter, tol, prior


def _pack(codes: torch.Tensor) -> torch.Tensor:
    N, Ld = codes.shape
    bits = torch.empty((N, 4), dtype=torch.int32, device=codes.device)
    L.call("rbvae_bern_pack", codes, N, Ld, bits)
    return bits


def pack_codes(codes: torch.Tensor) -> torch.Tensor:
    """The f32 device matrix [N, L] that encode(hard=True) and encode_frames return -> int32 [N, 4] on the device: bit l of a
    row is codes[i, l] > 0.5 (symbols.code_symbols' rule), stored in word l // 32 at position l % 32; bits from L upward are 0."""
    codes, _, _, _ = _checked(codes, 1, "pack_codes")
    return _pack(codes)


class MStep:
    """rbvae_bern_mstep's outputs and workspace for packed codes of N rows and L bits and K components; run(resp, state) fills
    them from resp [K, N]"""

    def __init__(self, bits, N, Ld, K, prior):
        f = lambda *s: torch.empty(s, dtype=torch.float64, device=bits.device)     # noqa: E731
        self.bits, self.N, self.Ld, self.K, self.prior = bits, N, Ld, K, prior
        self.weights, self.logw, self.theta, self.logt, self.logf = f(K), f(K), f(K, Ld), f(K, Ld), f(K, Ld)
        self.ws = f(L.query("rbvae_bern_ws_bytes", N, Ld, K) // 8)

    def run(self, resp, state=None):
        L.call("rbvae_bern_mstep", self.bits, self.N, self.Ld, resp, self.K, self.prior, self.weights, self.logw, self.theta,
               self.logt, self.logf, self.ws, state)


def bmm(codes: torch.Tensor, n_components: int, init: Union[str, torch.Tensor, np.ndarray] = "kmeans", max_iter: int = 100,
        tol: float = 1e-3, prior: float = 1.0, seed: int = 42) -> BMMResult:
    """The Bernoulli mixture of an f32 device matrix of hard codes [N, L] (a value > 0.5 is a set bit).  init: "kmeans"
    (symbols.kmeans(codes, K, seed=seed).labels) or an integer label vector [N] in [0, K).  The loop and the stop rule are
    mixture.gmm's: one M-step on the one-hot start, then E, M and the decision on the device (|lower bound - previous| < tol ->
    converged; else n_iter = max_iter -> not converged), ENQUEUE iterations enqueued per read of the state.  prior > 0 is the
    pseudo-count of a set and of a cleared bit in every state.  The labels come from one more E-step with the final parameters."""
    max_iter, tol, prior = _arguments(max_iter, tol, prior, init)
    codes, N, Ld, K = _checked(codes, n_components, "bmm")
    dev = codes.device
    lab = mixture.start_labels(codes, K, init, seed)
    bits = _pack(codes)
    resp = torch.zeros((K, N), dtype=torch.float64, device=dev)
    resp.scatter_(0, lab.view(1, N), 1.0)
    m = MStep(bits, N, Ld, K, prior)
    lognorm = torch.empty(N, dtype=torch.float64, device=dev)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    lb = torch.full((1,), float("-inf"), dtype=torch.float64, device=dev)
    history = torch.zeros(max_iter, dtype=torch.float64, device=dev)
    m.run(resp)

    def iteration(it):
        L.call("rbvae_bern_estep", bits, N, Ld, m.logt, m.logf, m.logw, K, resp, lognorm, None, state)
        m.run(resp, state)
        L.call("rbvae_gmm_decide", lognorm, N, tol, max_iter, lb, history, state)

    n_iter, why, _ = run_until_done(iteration, state, max_iter)
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    L.call("rbvae_bern_estep", bits, N, Ld, m.logt, m.logf, m.logw, K, None, lognorm, labels, None)
    bounds = history[:n_iter].cpu().numpy()
    return BMMResult(m.weights, m.theta, m.logt, m.logf, m.logw, int(n_iter), why == 1, float(bounds[-1]), bounds, labels)


def _same_bits(fit, codes, what, chain=False):
    K, Lf = fit.probs.shape
    if isinstance(codes, torch.Tensor) and codes.dim() == 2 and codes.shape[1] != Lf:
        raise ValueError(f"{what}: the codes have {codes.shape[1]} columns, the fit {Lf}")
    return _checked(codes, K, what, chain)


def _bmm_estep(fit: BMMResult, codes, what, want_resp=False, want_label=False):
    codes, N, Ld, K = _same_bits(fit, codes, what)
    dev = codes.device
    resp = torch.empty((K, N), dtype=torch.float64, device=dev) if want_resp else None
    label = torch.empty(N, dtype=torch.int32, device=dev) if want_label else None
    lognorm = torch.empty(N, dtype=torch.float64, device=dev)
    L.call("rbvae_bern_estep", _pack(codes), N, Ld, fit.log_probs, fit.log_1m_probs, fit.log_weights, K, resp, lognorm, label,
           None)
    return resp, lognorm, label


def bmm_predict_proba(fit: BMMResult, codes: torch.Tensor) -> torch.Tensor:
    """f64 [N, K] on the device: every row's responsibilities (a view of the kernel's component-major [K, N])"""
    return _bmm_estep(fit, codes, "bmm_predict_proba", want_resp=True)[0].t()


def bmm_predict(fit: BMMResult, codes: torch.Tensor) -> torch.Tensor:
    """int32 [N] on the device: the component with the largest weighted log-probability, ties to the lower"""
    return _bmm_estep(fit, codes, "bmm_predict", want_label=True)[2]


def bmm_score_samples(fit: BMMResult, codes: torch.Tensor) -> torch.Tensor:
    """f64 [N] on the device: each row's log-likelihood under the mixture"""
    return _bmm_estep(fit, codes, "bmm_score_samples")[1]


def bmm_score(fit: BMMResult, codes: torch.Tensor) -> float:
    """the mean of bmm_score_samples, added on the device in rbvae_gmm_decide's order"""
    return mixture._mean_in_order(bmm_score_samples(fit, codes))


def bmm_n_parameters(K: int, Ld: int) -> int:
    """the free parameters of a Bernoulli mixture: K L bit probabilities and K - 1 weights"""
    return K * Ld + K - 1


def bmm_bic(fit: BMMResult, codes: torch.Tensor) -> float:
    """-2 score(codes) N + p log N"""
    return mixture.criteria(bmm_score(fit, codes), codes.shape[0], bmm_n_parameters(*fit.probs.shape))[0]


def bmm_aic(fit: BMMResult, codes: torch.Tensor) -> float:
    """-2 score(codes) N + 2 p"""
    return mixture.criteria(bmm_score(fit, codes), codes.shape[0], bmm_n_parameters(*fit.probs.shape))[1]


def bmm_select(codes: torch.Tensor, ks: Sequence[int], criterion: str = "bic", seed: int = 42, **fit_kwargs):
    """mixture.select with bmm, bmm_score and bmm_n_parameters -> (table: a list of {"K", "n_iter", "converged", "score", "bic",
    "aic"} in ks' order, the chosen K (the lowest criterion, a tie to the smaller K), its BMMResult)"""
    return mixture.select(codes, ks, criterion, lambda K: bmm(codes, K, seed=seed, **fit_kwargs),
                          lambda fit: bmm_score(fit, codes), bmm_n_parameters)


def _emit(buf, bits, N, Ld, K, logt, logf, state=None):
    L.call("rbvae_bern_emit", bits, N, Ld, logt, logf, K, buf.logb, buf.rowmax, buf.e, state)


def bhmm(codes: torch.Tensor, n_states: int, init: Union[str, torch.Tensor, np.ndarray] = "kmeans", max_iter: int = 100,
         tol: float = 1e-3, prior: float = 1.0, seed: int = 42, block_rows: Optional[int] = None,
         lengths: Optional[Sequence[int]] = None) -> BHMMResult:
    """Baum-Welch with Bernoulli emissions for an f32 device matrix of hard codes [N, L] whose rows are one sequence in time
    order, or with lengths several, stacked (hmm.hmm's: no transition across a boundary, pi from every first row).  It is
    hmm.hmm's iteration -- the emissions, the recursions and the posterior under the current parameters, then pi
    and A (rbvae_hmm_posterior), theta from the posterior (rbvae_bern_mstep; its weights are unused) and the mixture's decision
    on the device -- with the same start (theta from the labelling's one-hot posterior, A_ij = (n_ij + 1) / (sum_j n_ij + K),
    pi = 1 / K), the same "degenerate" ending and the same final pass for the posterior and the Viterbi path."""
    max_iter, tol, prior = _arguments(max_iter, tol, prior, init)
    codes, N, Ld, K = _checked(codes, n_states, "bhmm", chain=True)
    dev = codes.device
    R = _block_rows(block_rows)
    lab = mixture.start_labels(codes, K, init, seed)
    bits = _pack(codes)
    plan = _plan(lengths, N, R, dev, "bhmm")
    buf = _Buffers(N, K, R, dev, plan)
    buf.gamma.zero_()
    buf.gamma.scatter_(0, lab.view(1, N), 1.0)
    m = MStep(bits, N, Ld, K, prior)                        # its weights are unused
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    lb = torch.full((1,), float("-inf"), dtype=torch.float64, device=dev)
    history = torch.zeros(max_iter, dtype=torch.float64, device=dev)
    m.run(buf.gamma)
    A = _initial_transitions(lab, K, plan)
    pi = torch.full((K,), 1.0 / K, dtype=torch.float64, device=dev)

    def iteration(it):
        _emit(buf, bits, N, Ld, K, m.logt, m.logf, state)
        buf.recursions(pi, A, state)
        buf.posterior(A, A, pi, state)
        m.run(buf.gamma, state)
        L.call("rbvae_gmm_decide", buf.ll, N, tol, max_iter, lb, history, state)

    n_iter, why, degenerate = run_until_done(iteration, state, max_iter, also_stop=lambda: int(buf.status[0]) != 0)
    scratch_A, scratch_pi = torch.empty_like(A), torch.empty_like(pi)
    _emit(buf, bits, N, Ld, K, m.logt, m.logf)
    buf.recursions(pi, A)
    buf.posterior(A, scratch_A, scratch_pi)
    path, score, *scores = _viterbi(buf.logb, N, K, pi, A, plan)
    lls = history[:max(n_iter, 1)].cpu().numpy()
    reason = "degenerate" if degenerate else ("converged" if why == 1 else "max_iter")
    return BHMMResult(pi, A, m.theta, m.logt, m.logf, int(n_iter), reason == "converged", reason, float(lls[-1]), lls,
                      buf.gamma.t(), path, score, *((plan.lengths, scores[0]) if plan is not None else ()))


def _bhmm_estep(fit: BHMMResult, codes, what, posterior=False, lengths=None):
    codes, N, Ld, K = _same_bits(fit, codes, what, chain=True)
    R = _block_rows(None)
    buf = _Buffers(N, K, R, codes.device, _plan(lengths, N, R, codes.device, what))
    _emit(buf, _pack(codes), N, Ld, K, fit.log_probs, fit.log_1m_probs)
    if posterior is not None:
        buf.recursions(fit.startprob, fit.transmat)
    if posterior:
        buf.posterior(fit.transmat, torch.empty_like(fit.transmat), torch.empty_like(fit.startprob))
    return buf


def bhmm_score_samples(fit: BHMMResult, codes: torch.Tensor, lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
    """f64 [N] on the device: ll_t = log p(x_t | x_0 .. x_(t-1)), the earlier rows of its own sequence; a sequence's sum is its
    log-likelihood"""
    return _bhmm_estep(fit, codes, "bhmm_score_samples", lengths=lengths).ll


def bhmm_score(fit: BHMMResult, codes: torch.Tensor, lengths: Optional[Sequence[int]] = None) -> float:
    """the mean per-row log-likelihood of the sequence (or sequences), added on the device in rbvae_gmm_decide's order"""
    return mixture._mean_in_order(bhmm_score_samples(fit, codes, lengths))


def bhmm_predict(fit: BHMMResult, codes: torch.Tensor, lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
    """int32 [N] on the device: the Viterbi path of the sequence (of every sequence)"""
    buf = _bhmm_estep(fit, codes, "bhmm_predict", posterior=None, lengths=lengths)
    return _viterbi(buf.logb, buf.N, buf.K, fit.startprob, fit.transmat, buf.plan)[0]


def bhmm_predict_proba(fit: BHMMResult, codes: torch.Tensor, lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
    """f64 [N, K] on the device: the smoothed posterior of the sequence (of every sequence)"""
    return _bhmm_estep(fit, codes, "bhmm_predict_proba", posterior=True, lengths=lengths).gamma.t()


def bhmm_n_parameters(K: int, Ld: int) -> int:
    """K - 1 start probabilities, K (K - 1) transition probabilities and K L bit probabilities"""
    return (K - 1) + K * (K - 1) + K * Ld


def bhmm_bic(fit: BHMMResult, codes: torch.Tensor, lengths: Optional[Sequence[int]] = None) -> float:
    """-2 score(codes) N + p log N"""
    return mixture.criteria(bhmm_score(fit, codes, lengths), codes.shape[0], bhmm_n_parameters(*fit.probs.shape))[0]


def bhmm_aic(fit: BHMMResult, codes: torch.Tensor, lengths: Optional[Sequence[int]] = None) -> float:
    """-2 score(codes) N + 2 p"""
    return mixture.criteria(bhmm_score(fit, codes, lengths), codes.shape[0], bhmm_n_parameters(*fit.probs.shape))[1]


def bhmm_select(codes: torch.Tensor, ks: Sequence[int], criterion: str = "bic", seed: int = 42,
                lengths: Optional[Sequence[int]] = None, **fit_kwargs):
    """mixture.select with bhmm, bhmm_score and bhmm_n_parameters -> (table, the chosen K, its BHMMResult)"""
    if lengths is not None:
        fit_kwargs["lengths"] = lengths
    return mixture.select(codes, ks, criterion, lambda K: bhmm(codes, K, seed=seed, **fit_kwargs),
                          lambda fit: bhmm_score(fit, codes, lengths), bhmm_n_parameters)


@torch.no_grad()
def latent_code_models(model, x: torch.Tensor, frame_indices: Sequence[int], flags: Sequence[int],
                       n_states: Optional[int] = None, ks: Optional[Sequence[int]] = None, tolerance: int = 2,
                       criterion: str = "bic", projections: Optional[dict] = None, temperature: float = 0.2,
                       noise_ratio: float = 0.3, u=None, max_iter: int = 100, tol: float = 1e-3, prior: float = 1.0,
                       seed: int = 42) -> dict:
    """Both models of the script's hard codes in one call: x [F, C, H, W] frames (or latents) on the device in time order,
    encoded by _latents.encode_frames' hard pass (projections["latents"] serves as the soft latents when present); the states
    are data.assign_label(frame_indices[f], flags) and n_states defaults to their number, len(flags) + 1.  Both fits start from
    symbols.kmeans' labelling of the codes.
    -> {"codes", "labels" (the states), "bmm": BMMResult, "bhmm": BHMMResult, "bmm_agreement", "bhmm_agreement" (of the Viterbi
        path) and "kmeans_agreement": clustering_agreement against the states, "prototypes" bool [K, L] and "bit_reliability" f64
        [K, L] of the hidden Markov model, "change_points" of the Viterbi path, "boundaries": segments.boundary_agreement of them
        against the positions where the state changes, at `tolerance`, "dwell": f64 [K] on the host, 1 / (1 - A_kk), and with ks
        given "selection": bmm_select's (table, chosen K, fit)}"""
    from .segments import boundary_agreement
    labels = frame_labels(frame_indices, flags, frame_count(x))
    S = len(flags) + 1
    K = S if n_states is None else int(n_states)
    _, codes = encode_frames(model, x, hard=True, latents=projections.get("latents") if projections is not None else None,
                             temperature=temperature, noise_ratio=noise_ratio, u=u)
    kw = dict(max_iter=max_iter, tol=tol, prior=prior)
    start = symbols.kmeans(codes, K, seed=seed).labels
    mix = bmm(codes, K, init=start, seed=seed, **kw)
    chain = bhmm(codes, K, init=start, seed=seed, **kw)
    cps = change_points(chain.path)
    with np.errstate(divide="ignore"):
        dwell = 1.0 / (1.0 - torch.diagonal(chain.transmat).cpu().numpy())
    out = {"codes": codes, "labels": labels, "bmm": mix, "bhmm": chain,
           "bmm_agreement": symbols.clustering_agreement(labels, mix.labels, S, K),
           "bhmm_agreement": symbols.clustering_agreement(labels, chain.path, S, K),
           "kmeans_agreement": symbols.clustering_agreement(labels, start, S, K), "prototypes": chain.probs > 0.5,
           "bit_reliability": torch.maximum(chain.probs, 1.0 - chain.probs), "change_points": cps,
           "boundaries": boundary_agreement(cps, change_points(labels), tolerance), "dwell": dwell}
    if ks is not None:
        out["selection"] = bmm_select(codes, ks, criterion=criterion, seed=seed, **kw)
    return out
