"""Reference and element-wise bounds for the linear probe tests (csrc/probe.hip, probe.py).

restate() is the probe's formulation (probe.py's docstring; the reference's scikit-learn calls at
scripts/evaluation/linear_projection_eval/linear_regression_eval.py:114-144) in numpy, float64 inputs with
numpy.longdouble sums, written independently of the package.  tests/golden/linear_probe.npz pins it to scikit-learn.

The bounds follow tests/_bounds.py: u = 2^-53 is the unit roundoff of f64, a sum of n terms in ANY order is off by at
most (n - 1) u sum |terms| (recursive summation, first order), every bound carries a factor 2 of margin over that and
uses the term count of its own sum; nothing here was chosen by looking at device output.
  C = B^T (Y[rows] - y0)   the differences are exact, each product rounds once (or not at all inside a matrix-core fma
                           chain) and n_rows terms are added: |got - ref| <= 2 n_rows u S + tiny, S = sum |B| |y - y0|
  intercept                (C[L] - sum_l mean_x[l] C[l]) + y0 from the device's own C: L products, L + 2 additions:
                           <= 2 (L + 2) u (|C[L]| + sum |mean_x[l] C[l]| + |y0|)
  pass-2 sums              from the device's own W and intercept, so the conditioning of the fit stays out: per row the
                           prediction intercept + sum_l x_l W_l (L + 1 terms) and e = y - prediction are off by
                           delta_r <= (L + 2) u (|intercept| + sum |x_l W_l| + |y|); then, over m rows,
                             sum e, sum |e|:  2 (sum delta_r + m u sum |e_r|)
                             sum e^2:         2 (sum (2 |e_r| delta_r + delta_r^2) + (m + 1) u sum e_r^2)
                             sum d, sum d^2:  d is exact: 2 m u sum |d_r|, 2 (m + 1) u sum d_r^2
"""
import math

import numpy as np

U = 2.0 ** -53
TINY = 1e-300
LD = np.longdouble
CASES = ("full_rank", "dead_bits", "under_determined", "large_n")     # the four scikit-learn cases of the fixture
CONST_CASE = "constant_columns"


def target_values(Y):
    """float64 values of targets as the kernels read them: u8 -> ToTensor's f32 v / 255 widened; f32 widened.
    [N, ...] -> [N, P] in memory order."""
    Y = np.asarray(Y)
    if Y.dtype == np.uint8:
        v = Y.astype(np.float32) / np.float32(255.0)
    else:
        v = Y.astype(np.float32)
    return v.astype(np.float64).reshape(Y.shape[0], -1)


def chw(a, hwc):
    """[..., P] in NHWC memory order -> the reference's CHW flatten order"""
    H, W, C = hwc
    lead = a.shape[:-1]
    return np.moveaxis(a.reshape(*lead, H, W, C), -1, -3).reshape(*lead, H * W * C)


def split(n, test_size=0.2, seed=42):
    n_test = int(math.ceil(test_size * n))
    perm = np.random.RandomState(seed).permutation(n)
    return perm[n_test:], perm[:n_test]


def singular_values(X_train):
    X = np.asarray(X_train, dtype=np.float64)
    return np.linalg.svd(X - X.mean(axis=0), compute_uv=False)


def assert_rank_gap(X_train, what=""):
    """Every singular value of the centred train embeddings is <= 1e-13 s_max or >= 1e-3 s_max: the rank cut then does
    not depend on the host LAPACK.  Returns the number kept."""
    s = singular_values(X_train)
    small, large = s <= 1e-13 * s[0], s >= 1e-3 * s[0]
    assert bool(np.all(small | large)), f"{what}: singular values inside the gap: {s[~(small | large)] / s[0]}"
    return int(large.sum())


def factor(X_train, rcond=None):
    """B [n, L + 1] and mean_x [L] (probe.py's fit factor, restated)"""
    X = np.asarray(X_train, dtype=np.float64)
    n, Ld = X.shape
    mean_x = (X.astype(LD).sum(axis=0) / n).astype(np.float64)
    Uu, s, Vt = np.linalg.svd(X - mean_x, full_matrices=False)
    if rcond is None:
        rcond = max(n, Ld) * 2.0 ** -52
    sinv = np.array([1.0 / v if v > rcond * s[0] else 0.0 for v in s])
    return np.concatenate([(Uu * sinv) @ Vt, np.full((n, 1), 1.0 / n)], axis=1), mean_x


def scores(se, see, sd, sdd, m):
    """per-target r2 and explained variance from the pass-2 sums, scikit-learn's force_finite rule"""
    sstot = sdd - sd * sd / m
    num_ev, den_ev = see / m - (se / m) ** 2, sstot / m
    with np.errstate(divide="ignore", invalid="ignore"):
        r2 = np.where(sstot != 0, 1 - see / sstot, np.where(see != 0, 0.0, 1.0))
        evs = np.where(den_ev != 0, 1 - num_ev / den_ev, np.where(num_ev != 0, 0.0, 1.0))
    return r2, evs, sstot


def restate(X, Yv, train, test, rcond=None):
    """The whole probe on float64 target values Yv [N, P]: dict of coef [P, L], intercept [P], r2, mse, mae, evs,
    per-target r2 / evs and n_constant (all float64)."""
    X = np.asarray(X, dtype=np.float64)
    B, mean_x = factor(X[train], rcond)
    Ld, m = X.shape[1], len(test)
    D = (Yv[train] - Yv[train[0]]).astype(LD)               # exact differences
    C = B.astype(LD).T @ D
    W = C[:Ld]
    icpt = (C[Ld] - mean_x.astype(LD) @ W) + Yv[train[0]]
    e = Yv[test] - (icpt + X[test].astype(LD) @ W)
    d = (Yv[test] - Yv[test[0]]).astype(LD)
    se, see, sae, sd, sdd = e.sum(0), (e * e).sum(0), np.abs(e).sum(0), d.sum(0), (d * d).sum(0)
    r2, evs, sstot = scores(se, see, sd, sdd, LD(m))
    P = Yv.shape[1]
    f = np.float64
    return {"coef": W.T.astype(f), "intercept": icpt.astype(f), "r2": f(r2.sum() / P), "evs": f(evs.sum() / P),
            "mse": f(see.sum() / (LD(m) * P)), "mae": f(sae.sum() / (LD(m) * P)), "r2_per_target": r2.astype(f),
            "evs_per_target": evs.astype(f), "n_constant": int((sstot == 0).sum())}


# ---- element-wise references and bounds of the kernels --------------------------------------------------------------

def xty_ref(B, Yv, rows, row0):
    """(ref, bound) of C = B^T (Yv[rows] - Yv[row0]); rows outside [0, N) contribute nothing."""
    rows = np.asarray(rows)
    ok = (rows >= 0) & (rows < Yv.shape[0])
    D = (Yv[rows[ok]] - Yv[row0]).astype(LD)
    Bk = np.asarray(B, dtype=np.float64)[ok].astype(LD)
    ref = Bk.T @ D
    S = np.abs(Bk).T @ np.abs(D)
    return ref.astype(np.float64), (2 * len(rows) * U * S + TINY).astype(np.float64)


def intercept_ref(C, mean_x, y0):
    """(ref, bound) of (C[L] - sum_l mean_x[l] C[l]) + y0 from the device's C"""
    Ld = len(mean_x)
    Cl, mx = np.asarray(C, dtype=np.float64).astype(LD), np.asarray(mean_x, dtype=np.float64).astype(LD)
    ref = (Cl[Ld] - mx @ Cl[:Ld]) + y0
    S = np.abs(Cl[Ld]) + np.abs(mx) @ np.abs(Cl[:Ld]) + np.abs(y0)
    return ref.astype(np.float64), (2 * (Ld + 2) * U * S + TINY).astype(np.float64)


def residual_ref(Xr, W, icpt, Yv, rows, row0):
    """(ref [5, P], bound [5, P]) of sum e, sum e^2, sum |e|, sum d, sum d^2 from the device's W [L, P] and intercept;
    Xr [n, L] holds the embedding of rows[r] in row r; rows outside [0, N) contribute nothing."""
    rows = np.asarray(rows)
    ok = (rows >= 0) & (rows < Yv.shape[0])
    x = np.asarray(Xr, dtype=np.float64)[ok].astype(LD)
    Wl, ic = np.asarray(W, dtype=np.float64).astype(LD), np.asarray(icpt, dtype=np.float64).astype(LD)
    y = Yv[rows[ok]].astype(LD)
    Ld, m = x.shape[1], int(ok.sum())
    e = y - (ic + x @ Wl)
    d = y - Yv[row0]
    delta = (Ld + 2) * U * (np.abs(ic) + np.abs(x) @ np.abs(Wl) + np.abs(y))
    ae = np.abs(e)
    ref = np.stack([e.sum(0), (e * e).sum(0), ae.sum(0), d.sum(0), (d * d).sum(0)])
    b_e = 2 * (delta.sum(0) + m * U * ae.sum(0))
    bnd = np.stack([b_e, 2 * ((2 * ae * delta + delta * delta).sum(0) + (m + 1) * U * (e * e).sum(0)), b_e,
                    2 * m * U * np.abs(d).sum(0), 2 * (m + 1) * U * (d * d).sum(0)])
    return ref.astype(np.float64), (bnd + TINY).astype(np.float64)


def within(got, ref, bnd, what):
    """Assert |got - ref| <= bnd element-wise (NaN fails); returns the worst |err| / bound."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref)
    ratio = np.where(np.isnan(err), np.inf, err / bnd)
    bad = ~(err <= bnd)
    if bad.any():
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the bound; worst |err|/bound = "
                             f"{ratio[i]:.3g} at {i}: got {got[i]!r}, ref {ref[i]!r}, bound {bnd[i]:.3g}")
    return float(ratio.max()) if ratio.size else 0.0


# ---- the fixture's synthetic cases (tools/make_probe_golden.py) ------------------------------------------------------

def make_case(name, seed=20261017):
    """-> (X f32 [N, L], Y u8 [N, h, h, 3]): embeddings and frames that depend on them linearly plus noise."""
    rng = np.random.default_rng([seed, sorted(CASES + (CONST_CASE,)).index(name)])
    N, Ld, h = {"full_rank": (128, 32, 16), "dead_bits": (128, 32, 16), "under_determined": (24, 32, 16),
                "large_n": (2000, 32, 8), CONST_CASE: (128, 32, 16)}[name]
    if name == "dead_bits":
        X = (rng.random((N, Ld)) < 0.5).astype(np.float32)
        X[:, 3], X[:, 17] = 0.0, 1.0                        # two constant bits
        X[:, 29] = X[:, 5]                                  # one duplicated bit
    else:
        X = (np.round(rng.standard_normal((N, Ld)) * 16.0) / 16.0).astype(np.float32)    # multiples of 1/16: compressible
    P = h * h * 3
    G = rng.standard_normal((Ld, P)) * (18.0 / np.sqrt(Ld))
    Y = 128.0 + (X.astype(np.float64) - X.mean(0)) @ G + rng.normal(0.0, 12.0, (N, P))
    step = 3 if name == "under_determined" else 17           # few levels keep the file small; the 5 test rows of the
    Y = (np.clip(np.round(Y / step), 0, 255 // step) * step).astype(np.uint8).reshape(N, h, h, 3)   # small case need more
    if name == CONST_CASE:
        flat = Y.reshape(N, -1)
        flat[:, [0, 7, 100, 501, P - 1]] = np.array([255, 1, 77, 128, 200], dtype=np.uint8)   # non-zero constants
    return X, Y
