"""CPU: the host side of the linear probe (probe.py split_indices / fit_factor), the numpy restatement the GPU tests
use (tests/_probe_ref.py) and the ABI, against the scikit-learn fixture tests/golden/linear_probe*.npz
(tools/make_probe_golden.py: the reference's calls at linear_regression_eval.py:117-144).

Tolerances.  Metrics: 1e-10 max(1, |ref|) for r2 / evs and 1e-10 ref for mse / mae, the gate of the GPU end-to-end test:
two f64 implementations agree to ~5e-16 while the reference's own f32 run sits >= 1e-9 (relative) away.  Coefficients:
two backward-stable least-squares solutions differ by O(n kappa u) of their scale; every fixture keeps only singular
values >= 1e-3 s_max (assert_rank_gap), so kappa <= 1e3 and 8 max(n, L) kappa 2^-53 (max |coef| + max |intercept|)
bounds the difference with room for the constants of either solver."""
import ctypes
import os

import numpy as np
import pytest

import _probe_ref as R
import sfv_amd as sfv

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(GOLD, "linear_probe.npz")))
    g.update({k: v for k, v in np.load(os.path.join(GOLD, "linear_probe_coef.npz")).items() if "/" in k})
    return g


def _gate(got, ref):
    """r2, mse, mae, evs against the fixture's f64 scikit-learn values; returns the distances"""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    lim = 1e-10 * np.array([max(1.0, abs(ref[0])), ref[1], ref[2], max(1.0, abs(ref[3]))])
    assert np.all(d <= lim), f"metric distances {d} above {lim}"
    return d


def _coef_bound(n, Ld, coef, icpt):
    return 8 * max(n, Ld) * 1e3 * R.U * (np.abs(coef).max() + np.abs(icpt).max())


@pytest.mark.parametrize("name", R.CASES + (R.CONST_CASE,))
def test_split_is_train_test_split(gold, name):
    train, test = sfv.probe.split_indices(len(gold[f"{name}/X"]), 0.2, 42)
    assert np.array_equal(train, gold[f"{name}/train"]) and np.array_equal(test, gold[f"{name}/test"])
    rt, rs = R.split(len(gold[f"{name}/X"]))
    assert np.array_equal(rt, train) and np.array_equal(rs, test)


def test_split_rejects_empty_sides():
    with pytest.raises(ValueError):
        sfv.probe.split_indices(1)
    with pytest.raises(ValueError):
        sfv.probe.split_indices(10, test_size=1.0)


@pytest.mark.parametrize("name", R.CASES + (R.CONST_CASE,))
def test_fixture_has_a_rank_gap(gold, name):
    kept = R.assert_rank_gap(gold[f"{name}/X"][gold[f"{name}/train"]], name)
    assert kept == int(gold[f"{name}/rank"])


@pytest.mark.parametrize("name", R.CASES)
def test_fit_factor_reproduces_sklearn_coefficients(gold, name):
    X, Y, train = gold[f"{name}/X"], gold[f"{name}/Y"], gold[f"{name}/train"]
    Yv = R.chw(R.target_values(Y), Y.shape[1:])
    B, mean_x = sfv.fit_factor(X[train])
    Ld = X.shape[1]
    assert B.shape == (len(train), Ld + 1) and B.dtype == np.float64 and mean_x.shape == (Ld,)
    C = B.T @ Yv[train]
    coef, icpt = C[:Ld].T, C[Ld] - mean_x @ C[:Ld]
    lim = _coef_bound(len(train), Ld, gold[f"{name}/coef"], gold[f"{name}/intercept"])
    dc, di = np.abs(coef - gold[f"{name}/coef"]).max(), np.abs(icpt - gold[f"{name}/intercept"]).max()
    print(f"{name}: |coef - sklearn| {dc:.3g}, |intercept - sklearn| {di:.3g}, bound {lim:.3g}")
    assert dc <= lim and di <= lim
    # the operator annihilates constants, which is why pass 1 needs no centring of the targets
    assert np.abs(B[:, :Ld].sum(axis=0)).max() <= 8 * len(train) * 1e3 * R.U * np.abs(B[:, :Ld]).max()


def test_fit_factor_rejects_bad_shapes():
    with pytest.raises(ValueError):
        sfv.fit_factor(np.zeros((4, 129)))
    with pytest.raises(ValueError):
        sfv.fit_factor(np.zeros((0, 3)))
    with pytest.raises(ValueError):
        sfv.fit_factor(np.zeros(5))


@pytest.mark.parametrize("name", R.CASES)
def test_restatement_reproduces_the_fixture(gold, name):
    X, Y = gold[f"{name}/X"], gold[f"{name}/Y"]
    r = R.restate(X, R.chw(R.target_values(Y), Y.shape[1:]), gold[f"{name}/train"], gold[f"{name}/test"])
    d = _gate([r["r2"], r["mse"], r["mae"], r["evs"]], gold[f"{name}/metrics_f64"])
    print(f"{name}: |restatement - sklearn f64| r2 {d[0]:.3g} mse {d[1]:.3g} mae {d[2]:.3g} evs {d[3]:.3g}")
    lim = _coef_bound(len(gold[f"{name}/train"]), X.shape[1], gold[f"{name}/coef"], gold[f"{name}/intercept"])
    assert np.abs(r["coef"] - gold[f"{name}/coef"]).max() <= lim
    assert np.abs(r["intercept"] - gold[f"{name}/intercept"]).max() <= lim
    assert r["n_constant"] == 0


def test_restatement_scores_constant_columns_exactly_one(gold):
    name = R.CONST_CASE
    X, Y = gold[f"{name}/X"], gold[f"{name}/Y"]
    r = R.restate(X, R.chw(R.target_values(Y), Y.shape[1:]), gold[f"{name}/train"], gold[f"{name}/test"])
    const = gold[f"{name}/constant_targets"]
    assert r["n_constant"] == len(const) == 5
    assert np.all(r["r2_per_target"][const] == 1.0) and np.all(r["evs_per_target"][const] == 1.0)
    assert np.all(r["coef"][const] == 0.0)
    rest = np.delete(np.stack([r["r2_per_target"], r["evs_per_target"]]), const, axis=1)
    ref = gold[f"{name}/per_target_f64"]
    assert np.all(np.abs(rest - ref) <= 1e-10 * np.maximum(1.0, np.abs(ref)))


@pytest.mark.parametrize("name", R.CASES)
def test_restatement_reproduces_live_sklearn(gold, name):
    pytest.importorskip("sklearn")
    from sklearn.linear_model import LinearRegression
    from sklearn.metrics import explained_variance_score, mean_absolute_error, mean_squared_error, r2_score
    from sklearn.model_selection import train_test_split
    X, Y = gold[f"{name}/X"].astype(np.float64), gold[f"{name}/Y"]
    Yv = R.chw(R.target_values(Y), Y.shape[1:])
    idx = np.arange(len(X))
    Xtr, Xte, ytr, yte, itr, ite = train_test_split(X, Yv, idx, test_size=0.2, random_state=42)
    model = LinearRegression().fit(Xtr, ytr)
    pred = model.predict(Xte)
    ref = np.array([r2_score(yte, pred, multioutput="uniform_average"), mean_squared_error(yte, pred),
                    mean_absolute_error(yte, pred), explained_variance_score(yte, pred, multioutput="uniform_average")])
    train, test = R.split(len(X))
    assert np.array_equal(train, itr) and np.array_equal(test, ite)
    r = R.restate(X, Yv, train, test)
    d = _gate([r["r2"], r["mse"], r["mae"], r["evs"]], ref)
    print(f"{name}: |restatement - live sklearn| {d}")


def test_bounds_hold_for_a_plain_f64_evaluation():
    """the bounds are not vacuous and not violated by numpy's own f64 arithmetic in another summation order"""
    rng = np.random.default_rng(5)
    Yv = R.target_values(rng.integers(0, 256, (40, 50), dtype=np.uint8))
    B = rng.standard_normal((37, 9))
    rows = rng.permutation(40)[:37]
    ref, bnd = R.xty_ref(B, Yv, rows, int(rows[0]))
    got = (B[::-1].T @ (Yv[rows[::-1]] - Yv[rows[0]]))
    assert R.within(got, ref, bnd, "numpy f64, reversed order") <= 1.0
    assert bnd.max() < 1e-12


def test_header_declares_and_library_exports_the_probe():
    L = sfv._lib
    protos = L.parse_header()
    names = ["rbvae_probe_xty", "rbvae_probe_xty_slabs", "rbvae_probe_xty_ws_bytes", "rbvae_probe_intercept",
             "rbvae_probe_residual_sums", "rbvae_probe_finish", "rbvae_probe_finish_parts"]
    assert not [n for n in names if n not in protos]
    raw = ctypes.CDLL(L.LIB_PATH)
    assert not [n for n in names if not hasattr(raw, n)]
    assert [a for _, a in protos["rbvae_probe_xty"][1]][-1] == "stream"
    # workspace query: no slabs while the target tiles fill the device, slabs for long row lists on few targets
    assert L.query("rbvae_probe_xty_ws_bytes", 102, 33, 196608) == 0
    s = L.query("rbvae_probe_xty_slabs", 600, 33, 200)
    assert s > 1 and L.query("rbvae_probe_xty_ws_bytes", 600, 33, 200) == s * 33 * 200 * 8
    src = open(L.HEADER).read()
    assert src.count("linear_regression_eval.py:1") >= 4


def test_probe_is_exported_like_robustness():
    for n in ("linear_probe", "frame_probe", "fit_factor", "ProbeResult"):
        assert hasattr(sfv, n)
    assert sfv.probe.split_indices is not sfv.split_indices


def test_cpu_targets_raise():
    import torch
    with pytest.raises(ValueError, match="GPU"):
        sfv.linear_probe(np.zeros((8, 2)), torch.zeros((8, 4, 4, 3), dtype=torch.uint8))
