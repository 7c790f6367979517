"""Reference and bounds for the Gaussian-mixture tests (csrc/gmm.hip, mixture.py).

An f64 numpy restatement of scikit-learn 1.7.2's GaussianMixture(covariance_type="diag", n_init=1) in the orders
include/rbvae_hip.h states, written independently of the package; tests/golden/gmm.npz (tools/make_gmm_golden.py) pins it to
scikit-learn.  Functions take a `defect` name: the restatement with one named mistake, which tests/test_gmm_cpu.py uses to
show that the check meant to catch that mistake does.

The forms are direct: lp_ik = logc_k - q_ik / 2 with q_ik = sum_l ((x_il - mu_kl) s_kl)^2, l ascending, and the variance is
centred on the new mean, var_kl = sum_i r_ki (x_il - mu_kl)^2 / nk_k + reg_covar; scikit-learn expands both squares, and
where variances reach 2e-6 its own cancellation shows as 3e-11 relative.  The start runs the one-hot responsibilities
through the M-step, so its weights are nk / sum nk where scikit-learn's initialisation has nk / N (K * 10 * 2^-52 apart).

Bounds.  u = 2^-53 is the f64 unit roundoff; every count is first order, each rounding taken at its full half ulp with the
same sign; the device's exp and log are taken as accurate to 2 ulp = 4 u relative (nobody measured that: the tests print
the worst error / bound of each quantity).  Nothing was chosen by looking at device output.  References are long double,
rounded to f64 for the comparison: every bound below carries one more u |ref| for that rounding (ROUND).
  q        per coordinate the difference rounds once, the product with s once (both doubled by the square) and the square
           once: 5 u; the L additions of non-negative terms L u: |got - ref| <= (L + 5) u q.
  lp       logc - q / 2 (the halving is exact) rounds once: b_lp = (L + 5) u q / 2 + u |lp|.
  lognorm  log-sum-exp moves by at most max_k |d lp_k| when lp moves: max_k b_lp.  Its own evaluation: a_k = lp_k - m rounds
           (u |a_k|, relative to e_k = exp(a_k)), exp 4 u, the K additions of positive terms K u: the sum S is off by
           (K + 4) u S + u sum_k e_k |a_k|; log turns that into (K + 4) u + u W, W = sum_k e_k |a_k| / S, and adds 4 u |log S|;
           m + log S rounds once:  b_ln = max_k b_lp + u (K + 4 + W + 4 |log S| + |lognorm|).
  resp     exp(lp_k - lognorm): the argument is off by b_lp_k + b_ln and rounds (u |lp_k - lognorm|), exp 4 u:
           b_r = resp_k (b_lp_k + b_ln + u |lp_k - lognorm| + 4 u) (+ 1e-300 for the subnormal range).
  label    equal wherever the runner-up's lp is more than the two bounds below the winner's (decided).
  nk       N terms in any order and the added 10 eps: N u nk.
  mean     each product r x rounds (u) and the N additions: (N + 1) u sum |r x| / nk; nk's own N u and the division's u on the
           quotient: b_mu = u ((N + 1) sum_i |r_ki x_il| / nk_k + (N + 1) |mu_kl|).
  var      against the long double sum centred on the DEVICE's mean: d = x - mu rounds once (2 u after the square), the
           square and the product once each, N additions: (N + 4) u v with v = var - reg_covar; nk (N u v), the division and
           the added reg_covar (u var each way): b_var = u ((2 N + 5) v + var).
  weights  nk_k / sum_k nk_k from the device's nk against the long double quotient of the long double nk: nk's N u, the K
           additions K u, the division u: (N + K + 1) u w; their sum is 1 within K ulp = 2 K u.
  s, logc  from the device's own variances and weights: s = 1 / sqrt(var) has two correctly rounded operations, 2 u s.  log
           4 u |log| each, the L additions L u sum |log s|, the two outer operations u each on values below
           |log w| + sum |log s| + c, the constant c = L / 2 log 2 pi u c:
           b_logc = u ((L + 4) sum_l |log s_kl| + 5 |log w_k| + 2 (|log w_k| + sum_l |log s_kl| + c) + c).
  lb       N terms in a fixed order: N u sum |lognorm| / N; the division and the reference's rounding: + 2 u |lb|.
"""
import numpy as np

from _projection_ref import TINY, U, rejects, within  # noqa: F401
from _spectral_ref import dots as _dots

LD = np.longdouble
GM_CHUNK = 4096                         # f64 values of means and precision roots per LDS chunk of rbvae_gmm_estep
NK_EPS = 10.0 * np.finfo(np.float64).eps
LOG_2PI = float(np.log(2.0 * np.pi))
KS, SEEDS = (2, 8, 17, 32), (0, 42)
DEFECTS = ("var_not_centred_on_new_mean", "nk_without_eps", "weights_over_n", "no_reg_covar", "lognorm_without_max",
           "logdet_sign", "lower_bound_after_mstep", "stop_on_relative_change", "n_iter_off_by_one", "tie_high",
           "bic_param_count_full")


def ROUND(ref):
    """the reference's own rounding to f64, and a floor for the subnormal range"""
    return U * np.abs(ref) + TINY


def chunk_components(L):
    return GM_CHUNK // (2 * ((L + 7) // 8 * 8))


def blocks_rows(N):
    """the M-step's row blocks: min(256, ceil(N / 256)) blocks of ceil(N / blocks) consecutive rows"""
    b = min(256, -(-N // 256))
    return b, -(-N // b)


def ws_bytes(N, L, K):
    return 16 * blocks_rows(N)[0] * K * (L + 1)


# ---- E-step ----------------------------------------------------------------------------------------------------------------

def quad(X, means, prec, dtype=np.float64):
    """[N, K]: q_ik = sum_l ((x_il - mu_kl) s_kl)^2, l ascending, every operation rounded in `dtype`"""
    X, means, prec = (np.asarray(a).astype(dtype) for a in (X, means, prec))
    Q = np.zeros((len(X), len(means)), dtype=dtype)
    for l in range(X.shape[1]):
        t = (X[:, None, l] - means[None, :, l]) * prec[None, :, l]
        Q += t * t
    return Q


def estep(X, means, prec, logc, defect=None, dtype=np.float64):
    """-> (lp [N, K], lognorm [N], resp [N, K], label [N]); defects "lognorm_without_max", "tie_high" """
    half = dtype(0.5)
    lp = np.asarray(logc).astype(dtype)[None, :] - half * quad(X, means, prec, dtype)
    K = lp.shape[1]
    m = np.zeros(len(lp), dtype=dtype) if defect == "lognorm_without_max" else lp.max(axis=1)
    S = np.zeros(len(lp), dtype=dtype)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        for k in range(K):
            S = S + np.exp(lp[:, k] - m)
        lognorm = m + np.log(S)
        resp = np.exp(lp - lognorm[:, None])
    label = (K - 1 - np.argmax(lp[:, ::-1], axis=1)) if defect == "tie_high" else np.argmax(lp, axis=1)
    return lp, lognorm, resp, label.astype(np.int32)


def estep_bounds(X, means, prec, logc):
    """long double references and the bounds of the docstring -> dict(lp, lognorm, resp, label, decided, b_lp, b_ln, b_r)"""
    L, K = np.asarray(X).shape[1], len(means)
    q = quad(X, means, prec, LD)
    lp, lognorm, resp, label = estep(X, means, prec, logc, dtype=LD)
    b_lp = ((L + 5) * U * 0.5 * q + U * np.abs(lp)).astype(np.float64)
    m = lp.max(axis=1)
    a = lp - m[:, None]
    e = np.exp(a)
    S = e.sum(axis=1)
    W = (e * np.abs(a)).sum(axis=1) / S
    b_ln = b_lp.max(axis=1) + U * (K + 4 + W + 4 * np.abs(np.log(S)) + np.abs(lognorm)).astype(np.float64)
    b_r = (resp * (b_lp + b_ln[:, None] + U * np.abs(lp - lognorm[:, None]) + 4 * U)).astype(np.float64)
    if K > 1:
        order = np.argsort(-lp, axis=1, kind="stable")
        rows = np.arange(len(lp))
        top, second = order[:, 0], order[:, 1]
        decided = (lp[rows, top] - lp[rows, second]).astype(np.float64) > b_lp[rows, top] + b_lp[rows, second]
    else:
        decided = np.ones(len(lp), dtype=bool)
    f = lambda v: v.astype(np.float64)  # noqa: E731
    return {"lp": f(lp), "lognorm": f(lognorm), "resp": f(resp), "label": label, "decided": decided,
            "b_lp": b_lp + ROUND(f(lp)), "b_ln": b_ln + ROUND(f(lognorm)), "b_r": b_r + ROUND(f(resp))}


# ---- M-step ----------------------------------------------------------------------------------------------------------------

def _block_sums(terms, N):
    """terms [N, ...] -> their sum: each block's rows added in ascending order from zero, the blocks in block order"""
    blocks, rows = blocks_rows(N)
    total = np.zeros(terms.shape[1:])
    for b in range(blocks):
        part = np.zeros(terms.shape[1:])
        for r in range(b * rows, min(N, (b + 1) * rows)):
            part = part + terms[r]
        total = total + part
    return total


def mstep(X, resp, reg_covar=1e-6, defect=None, old_means=None):
    """resp [N, K] -> (weights [K], means [K, L], covars [K, L], prec [K, L], logc [K], nk [K]).  defects:
    "var_not_centred_on_new_mean" (centred on old_means), "nk_without_eps", "weights_over_n", "no_reg_covar", "logdet_sign" """
    X = np.asarray(X).astype(np.float64)
    N, L = X.shape
    nk = _block_sums(resp, N) + (0.0 if defect == "nk_without_eps" else NK_EPS)
    with np.errstate(divide="ignore", invalid="ignore"):
        means = _block_sums(resp[:, :, None] * X[:, None, :], N) / nk[:, None]
        centre = old_means if defect == "var_not_centred_on_new_mean" else means
        d = X[:, None, :] - centre[None, :, :]
        covars = _block_sums(resp[:, :, None] * (d * d), N) / nk[:, None] + (0.0 if defect == "no_reg_covar" else reg_covar)
        tot = 0.0
        for k in range(len(nk)):
            tot = tot + nk[k]
        weights = nk / (N if defect == "weights_over_n" else tot)
        prec = 1.0 / np.sqrt(covars)
        logs = np.log(prec)
        t = np.zeros(len(nk))
        for l in range(L):
            t = t + logs[:, l]
        logc = (np.log(weights) + (-t if defect == "logdet_sign" else t)) - 0.5 * L * LOG_2PI
    return weights, means, covars, prec, logc, nk


def mstep_bounds(X, resp, reg_covar, dev_means, dev_covars, dev_weights, dev_nk=None):
    """long double references (resp [N, K] f64 as given) and the bounds of the docstring; the variance is centred on the
    device's means, prec and logc follow from the device's variances and weights"""
    Xl, R = np.asarray(X).astype(LD), np.asarray(resp).astype(LD)
    N, L = Xl.shape
    K = R.shape[1]
    nk = R.sum(axis=0) + LD(NK_EPS)
    sx = R.T @ Xl
    sax = np.abs(R).T @ np.abs(Xl)
    means = sx / nk[:, None]
    d = Xl[:, None, :] - np.asarray(dev_means).astype(LD)[None, :, :]
    v = np.einsum("ik,ikl->kl", R, d * d) / nk[:, None]
    covars = v + LD(reg_covar)
    weights = nk / nk.sum()
    dv, dw = np.asarray(dev_covars).astype(LD), np.asarray(dev_weights).astype(LD)
    prec = 1 / np.sqrt(dv)
    logs = np.log(prec)
    c = LD(0.5 * L) * LD(LOG_2PI)
    logc = np.log(dw) + logs.sum(axis=1) - c
    sal = np.abs(logs).sum(axis=1)
    f = lambda a: a.astype(np.float64)  # noqa: E731
    return {"nk": f(nk), "means": f(means), "covars": f(covars), "weights": f(weights), "prec": f(prec), "logc": f(logc),
            "b_nk": N * U * f(nk) + ROUND(f(nk)),
            "b_means": U * ((N + 1) * f(sax / nk[:, None]) + (N + 1) * np.abs(f(means))) + ROUND(f(means)),
            "b_covars": U * ((2 * N + 5) * f(v) + f(covars)) + ROUND(f(covars)),
            "b_weights": (N + K + 1) * U * f(weights) + ROUND(f(weights)), "b_prec": 2 * U * f(prec) + ROUND(f(prec)),
            "b_logc": U * ((L + 4) * f(sal) + 5 * np.abs(f(np.log(dw))) + 2 * (np.abs(f(np.log(dw))) + f(sal) + float(c))
                           + float(c)) + ROUND(f(logc))}


# ---- lower bound, the fit, the criteria --------------------------------------------------------------------------------------

def lower_bound(lognorm):
    """(sum_i lognorm_i) / N in rbvae_spectral_dots' two-stage order"""
    lognorm = np.asarray(lognorm, dtype=np.float64)
    return float(_dots(np.ones(len(lognorm)), lognorm)[0][0]) / len(lognorm)


def lower_bound_bound(lognorm):
    lognorm = np.asarray(lognorm, dtype=np.float64)
    N = len(lognorm)
    return N * U * np.abs(lognorm).sum() / N + 2 * U * abs(float(lognorm.astype(LD).sum() / N)) + TINY


def one_hot(labels, K):
    R = np.zeros((len(labels), K))
    R[np.arange(len(labels)), labels] = 1.0
    return R


def n_parameters(K, L, defect=None):
    """2 K L + K - 1; defect "bic_param_count_full": a full covariance's K L (L + 1) / 2 + K L + K - 1"""
    return K * L * (L + 1) // 2 + K * L + K - 1 if defect == "bic_param_count_full" else 2 * K * L + K - 1


def criteria(score, N, K, L, defect=None):
    p = n_parameters(K, L, defect)
    return -2.0 * score * N + p * np.log(N), -2.0 * score * N + 2.0 * p


def fit(X, labels, K, max_iter=100, tol=1e-3, reg_covar=1e-6, defect=None):
    """scikit-learn's fit_predict from the one-hot start -> dict(weights, means, covars, prec, logc, n_iter, converged,
    lower_bound, lower_bounds, labels, score_samples, score, bic, aic).  defects: mstep's and estep's, and
    "lower_bound_after_mstep" (the bound is taken with the new parameters), "stop_on_relative_change" (|change| < tol |lb|),
    "n_iter_off_by_one", "bic_param_count_full" """
    X = np.asarray(X).astype(np.float64)
    N, L = X.shape
    w, mu, var, s, logc, _ = mstep(X, one_hot(labels, K), reg_covar, defect, old_means=np.zeros((K, L)))
    prev, history, converged = -np.inf, [], False
    for it in range(1, max_iter + 1):
        _, lognorm, resp, _ = estep(X, mu, s, logc, defect)
        w, mu, var, s, logc, _ = mstep(X, resp, reg_covar, defect, old_means=mu)
        if defect == "lower_bound_after_mstep":
            lognorm = estep(X, mu, s, logc, defect)[1]
        lb = lower_bound(lognorm)
        history.append(lb)
        change = abs(lb - prev)
        if change < (tol * abs(lb) if defect == "stop_on_relative_change" else tol):
            converged = True
            break
        prev = lb
    _, lognorm, _, label = estep(X, mu, s, logc, defect)
    score = lower_bound(lognorm)
    bic, aic = criteria(score, N, K, L, defect)
    return {"weights": w, "means": mu, "covars": var, "prec": s, "logc": logc,
            "n_iter": it - (1 if defect == "n_iter_off_by_one" else 0), "converged": converged, "lower_bound": history[-1],
            "lower_bounds": np.array(history), "labels": label, "score_samples": lognorm, "score": score, "bic": bic, "aic": aic}


def choose(ks, values):
    """the K with the lowest criterion; a tie goes to the smaller K"""
    return min(zip(values, ks))[1]


GATES = {"lower_bound": 1e-10, "lower_bounds": 1e-10, "score_samples": 1e-10, "means": 1e-10, "weights": 1e-10,
         "covars_rel": 1e-8, "bic_rel": 1e-10, "aic_rel": 1e-10}


def against_fixture(got, gold, t):
    """the issue's gates of a fit (a dict as fit returns it) against the fixture's case t -> the list of quantities outside
    their gate (empty: all inside) and the differences"""
    diff = {"n_iter": abs(int(got["n_iter"]) - int(gold["n_iter_" + t])),
            "converged": int(bool(got["converged"]) != bool(gold["converged_" + t])),
            "predict": int((np.asarray(got["labels"]) != gold["predict_" + t]).sum()),
            "lower_bound": abs(got["lower_bound"] - float(gold["lower_bound_" + t])),
            "lower_bounds": (float(np.abs(got["lower_bounds"] - gold["lower_bounds_" + t]).max())
                             if len(got["lower_bounds"]) == len(gold["lower_bounds_" + t]) else np.inf),
            "score_samples": float(np.abs(got["score_samples"] - gold["score_samples_" + t]).max()),
            "means": float(np.abs(got["means"] - gold["means_" + t]).max()),
            "weights": float(np.abs(got["weights"] - gold["weights_" + t]).max()),
            "covars_rel": float(np.abs(got["covars"] / gold["covars_" + t] - 1.0).max()),
            "bic_rel": abs(got["bic"] / float(gold["bic_" + t]) - 1.0), "aic_rel": abs(got["aic"] / float(gold["aic_" + t]) - 1.0)}
    bad = [k for k, v in diff.items() if not v <= GATES.get(k, 0)]
    return bad, diff


# ---- the synthetic cases of the kernel tests -----------------------------------------------------------------------------------

def soft_rows(N, Ld, seed):
    r = np.random.RandomState(seed)
    return (1.0 / (1.0 + np.exp(-2.0 * r.randn(N, Ld)))).astype(np.float32)


ESTEP_CASES = [(1, 1, 1), (257, 50, 17), (300, 128, chunk_components(128) + 1), (300, 2, 256), (16385, 2, 3)]


def params_case(N, Ld, K, seed=0):
    """X f32 [N, L]; means (rows of X moved by f64 noise), variances in [0.01, 0.26], weights: no f32 values, so every
    operation rounds -> (X, means, prec, logc, weights, covars)"""
    r = np.random.RandomState(1000 * N + 10 * Ld + K + seed)
    X = soft_rows(N, Ld, N + Ld + K)
    means = X[r.randint(0, N, K)].astype(np.float64) + 0.05 * r.randn(K, Ld)
    covars = 0.01 + 0.25 * r.rand(K, Ld)
    w = 0.2 + r.rand(K)
    w /= w.sum()
    prec = 1.0 / np.sqrt(covars)
    logc = (np.log(w) + np.log(prec).sum(axis=1)) - 0.5 * Ld * LOG_2PI
    return X, means, prec, logc, w, covars


def resp_case(N, K, kind, seed=0):
    """[N, K] f64 responsibilities: "soft" (a softmax of noise), "one_hot", "empty" (component K // 2 without mass),
    "one" (component K // 2 holds every row)"""
    r = np.random.RandomState(seed + N + K)
    if kind == "one":
        R = np.zeros((N, K))
        R[:, K // 2] = 1.0
        return R
    if kind == "one_hot":
        return one_hot(r.randint(0, K, N), K)
    R = np.exp(3.0 * r.randn(N, K))
    if kind == "empty":
        R[:, K // 2] = 0.0
    return R / R.sum(axis=1, keepdims=True)
