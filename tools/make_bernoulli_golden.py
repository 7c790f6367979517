"""Writes tests/golden/bernoulli.npz from scikit-learn 1.7.2 alone: an independent statement of one M-step from one-hot
responsibilities and one E-step of the Bernoulli models (symbols-from-video_amd/bernoulli.py, tests/_bernoulli_ref.py).

    python tools/make_bernoulli_golden.py

The codes are a planted chain (tests/_bernoulli_ref.planted_chain draws the same numbers; the CPU test compares them): N = 600
codes of L = 32 bits from K = 5 prototypes, every bit flipped with probability 0.2, the chain staying with probability 0.9,
RandomState(1).  BernoulliNB(alpha=a).fit(X, states) is the M-step of the states' one-hot responsibilities with prior = a; its
joint log-likelihood and predict_proba on X are the E-step.  Arrays only:
    X uint8 [N, L], states int32 [N], alphas f64 [2]
    feature_log_prob_A f64 [K, L]   log theta             A = 0, 1: the index into alphas (1.0 and 0.25)
    class_log_prior_A f64 [K]       log(nk / N)
    joint_A f64 [N, K]              _joint_log_likelihood(X): the weighted log-probabilities lp
    predict_proba_A f64 [N, K]      the responsibilities
"""
import os

import numpy as np
import sklearn
from sklearn.naive_bayes import BernoulliNB

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
N, L, K, FLIP, STAY, SEED = 600, 32, 5, 0.2, 0.9, 1
ALPHAS = (1.0, 0.25)


def planted_chain(N, L, K, flip, stay, seed):
    r = np.random.RandomState(seed)
    proto = r.rand(K, L) < 0.5
    s = np.zeros(N, dtype=np.int64)
    for t in range(1, N):
        s[t] = s[t - 1] if r.rand() < stay else r.randint(K)
    return (proto[s] ^ (r.rand(N, L) < flip)).astype(np.uint8), s.astype(np.int32)


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    X, s = planted_chain(N, L, K, FLIP, STAY, SEED)
    assert len(np.unique(s)) == K
    out = {"X": X, "states": s, "alphas": np.array(ALPHAS)}
    X64 = X.astype(np.float64)
    for a, alpha in enumerate(ALPHAS):
        nb = BernoulliNB(alpha=alpha, binarize=None, force_alpha=True).fit(X64, s)
        out[f"feature_log_prob_{a}"], out[f"class_log_prior_{a}"] = nb.feature_log_prob_, nb.class_log_prior_
        out[f"joint_{a}"], out[f"predict_proba_{a}"] = nb._joint_log_likelihood(X64), nb.predict_proba(X64)
    path = os.path.join(GOLDEN, "bernoulli.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes; rows per state {np.bincount(s).tolist()}, "
          f"{int((nb.predict(X64) == s).sum())} of {N} rows predicted as planted")


if __name__ == "__main__":
    main()
