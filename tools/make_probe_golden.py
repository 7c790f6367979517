"""Write tests/golden/linear_probe.npz and tests/golden/linear_probe_coef.npz: the reference's scikit-learn calls
(scripts/evaluation/linear_projection_eval/linear_regression_eval.py:117-144) on small synthetic cases, so the probe
tests have a scikit-learn yardstick that needs no scikit-learn where they run.  Arrays and a version string only.

    python tools/make_probe_golden.py

Per case: X f32 [N, L], Y u8 [N, h, h, 3], the split, the four metrics of the float64 run (the float64 casts of X and of
ToTensor's f32 frames, flattened CHW as the script does) and of the script's own f32 run, and for the four scikit-learn
cases coef_ [P, L] / intercept_ [P] of the float64 run.  The fifth case has non-zero constant target columns; their
expected score is this project's defined 1.0 (scikit-learn's own answer for such a column depends on rounding), so it
stores the constant columns and scikit-learn's per-target scores of the other columns.  coef_ / intercept_ (f64, not
compressible) go to the second file, so that each file stays well below 1 MiB.
"""
import os
import sys

import numpy as np
import sklearn
from sklearn.linear_model import LinearRegression
from sklearn.metrics import explained_variance_score, mean_absolute_error, mean_squared_error, r2_score
from sklearn.model_selection import train_test_split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _probe_ref as R  # noqa: E402


def run(X, Yf, dtype):
    """the script's calls on arrays of `dtype`; Yf [N, P] f32 in CHW flatten order"""
    idx = np.arange(len(X))
    Xtr, Xte, ytr, yte, itr, ite = train_test_split(X.astype(dtype), Yf.astype(dtype), idx, test_size=0.2,
                                                    random_state=42)
    model = LinearRegression()
    model.fit(Xtr, ytr)
    pred = model.predict(Xte)
    met = np.array([r2_score(yte, pred, multioutput="uniform_average"), mean_squared_error(yte, pred),
                    mean_absolute_error(yte, pred), explained_variance_score(yte, pred, multioutput="uniform_average")],
                   dtype=np.float64)
    per = np.stack([r2_score(yte, pred, multioutput="raw_values"),
                    explained_variance_score(yte, pred, multioutput="raw_values")]).astype(np.float64)
    return met, per, model.coef_, model.intercept_, itr, ite


def main():
    out = {"sklearn_version": np.array(sklearn.__version__)}
    coefs = {"sklearn_version": np.array(sklearn.__version__)}
    for name in R.CASES + (R.CONST_CASE,):
        X, Y = R.make_case(name)
        hwc = Y.shape[1:]
        Yf = R.chw((Y.astype(np.float32) / np.float32(255.0)).reshape(len(Y), -1), hwc)      # ToTensor + flatten
        met64, per64, coef, icpt, itr, ite = run(X, Yf, np.float64)
        met32 = run(X, Yf, np.float32)[0]
        kept = R.assert_rank_gap(X[itr], name)
        out[f"{name}/X"], out[f"{name}/Y"] = X, Y
        out[f"{name}/train"], out[f"{name}/test"] = itr.astype(np.int64), ite.astype(np.int64)
        out[f"{name}/rank"] = np.array(kept)
        if name == R.CONST_CASE:
            const = np.nonzero((Yf == Yf[0]).all(axis=0))[0]
            assert const.size == 5 and (Yf[0, const] != 0).all()
            out[f"{name}/constant_targets"] = const.astype(np.int64)         # CHW positions
            out[f"{name}/per_target_f64"] = np.delete(per64, const, axis=1)
        else:
            assert (Yf[ite] != Yf[ite[0]]).any(axis=0).all(), f"{name}: a target is constant over the test rows"
            out[f"{name}/metrics_f64"], out[f"{name}/metrics_f32"] = met64, met32
            coefs[f"{name}/coef"], coefs[f"{name}/intercept"] = coef.astype(np.float64), icpt.astype(np.float64)
        print(name, "rank", kept, "f64", met64, "f32 - f64", met32 - met64)
    for fname, arrays in (("linear_probe.npz", out), ("linear_probe_coef.npz", coefs)):
        path = os.path.join(ROOT, "tests", "golden", fname)
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
