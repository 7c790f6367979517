"""GPU: the mixture kernels (csrc/gmm.hip) against long double references inside NaN guard bands (tests/_bounds.py's
buffers) -- resp, lognorm, the M-step's outputs and the lower bound element-wise within the bounds tests/_gmm_ref.py
derives, labels and the state exact -- and mixture.py end to end against the scikit-learn fixture tests/golden/gmm.npz
(tools/make_gmm_golden.py) at the gates of tests/test_gmm_cpu.py.

Measured on one MI355X (each test prints its worst |error| / bound): no undecided row on any E-step case and every label
equal; lognorm at most 0.17 and resp 0.21 of their bounds (both at (16 385, 2, 3); 0.03 to 0.06 on the cases of 50 and 128
values; 0.09 and 0.18 on the far row); nk 0.024, means 0.022, variances 0.024, weights 0.018, prec_chol 0.65 and logc 0.13
of theirs, the weights adding to 1 within 5.6e-16 at K = 256; the lower bound 0.001 of its bound and equal bit for bit to
the restatement's sum in the header's order.  On the eight fixture cases n_iter, converged and predict equal
scikit-learn's, lower_bound within 2.1e-14, its history within 4.9e-14, score_samples within 1.0e-11, means within 1.4e-14,
weights within 1.0e-15 (gates 1e-10), variances within 3.0e-11 relative (1e-8), BIC and AIC within 6.7e-15 relative (1e-10).
The 40 tests take about 3.5 s together; no case takes more than 0.4 s.
"""
import os

import numpy as np
import pytest
import torch

import _bounds as B
import _gmm_ref as R
import sfv_amd as sfv

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 4096
# _bounds.py carries the sentinels of the bf16 and f32 outputs; these kernels write f64 and int32
B.SENTINEL.setdefault(torch.float64, (torch.int64, 0x7FF8DEADDEADBEEF))
B.SENTINEL.setdefault(torch.int32, (torch.int32, -0x21524111))
KS, SEEDS = R.KS, R.SEEDS
call, query = sfv._lib.call, sfv._lib.query


def G(dtype, *shape):
    """shape elements of dtype inside GUARD sentinel elements on each side; .t is the tensor handed to the kernel"""
    g = B.GuardedFlat(int(np.prod(shape)), dtype, guard=GUARD)
    g.t = g.view.view(*shape)
    return g


def out(g, what):
    B.assert_guards(g, what)
    return g.t.cpu().numpy()


def untouched(g, what):
    B.assert_guards_where(g, torch.zeros(g.rows, dtype=torch.bool), what)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _state(*v):
    return torch.tensor(list(v) or [0, 0, 0, 0], dtype=torch.int32, device="cuda")


def bits(a):
    return np.asarray(a).view(np.int64) if np.asarray(a).dtype == np.float64 else np.asarray(a)


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(HERE, "golden", "gmm.npz")))
    g["X"] = np.load(os.path.join(HERE, "golden", "latent_scores.npz"))["X"]
    g["Xd"] = _dev(g["X"])
    return g


# ---- E-step ------------------------------------------------------------------------------------------------------------------

def _estep(X, means, prec, logc, want_resp=True, want_label=True, state=None):
    N, Ld = X.shape
    K = len(means)
    resp, lognorm, label = G(torch.float64, K, N), G(torch.float64, N), G(torch.int32, N)
    call("rbvae_gmm_estep", _dev(X), N, Ld, _dev(means), _dev(prec), _dev(logc), K, resp.t if want_resp else None, lognorm.t,
         label.t if want_label else None, state)
    what = f"({N}, {Ld}, {K})"
    if not want_resp:
        untouched(resp, "resp " + what)
    if not want_label:
        untouched(label, "label " + what)
    return (out(resp, "resp " + what).T if want_resp else None, out(lognorm, "lognorm " + what),
            out(label, "label " + what) if want_label else None)


def _check_estep(X, means, prec, logc, what):
    ref = R.estep_bounds(X, means, prec, logc)
    resp, lognorm, label = _estep(X, means, prec, logc)
    wl = R.within(lognorm, ref["lognorm"], ref["b_ln"], "lognorm " + what)
    wr = R.within(resp, ref["resp"], ref["b_r"], "resp " + what)
    assert int((~ref["decided"]).sum()) == 0
    assert np.array_equal(label, ref["label"])
    print(f"E-step {what}: 0 undecided rows, worst |err|/bound lognorm {wl:.3g}, resp {wr:.3g}")
    return ref, resp, lognorm, label


@pytest.mark.parametrize("N,Ld,K", R.ESTEP_CASES)
def test_estep(N, Ld, K):
    X, means, prec, logc, _, _ = R.params_case(N, Ld, K)
    assert query("rbvae_gmm_ok", N, Ld, K) == 1
    if Ld == 128:                                           # 17 components just cross one LDS chunk
        assert query("rbvae_gmm_chunk_components", Ld) == R.chunk_components(Ld) == K - 1
    ref, resp, lognorm, label = _check_estep(X, means, prec, logc, f"({N}, {Ld}, {K})")
    resp2, lognorm2, label2 = _estep(X, means, prec, logc, state=_state())
    assert np.array_equal(bits(resp), bits(resp2)) and np.array_equal(bits(lognorm), bits(lognorm2)), "two runs differ"
    assert np.array_equal(label, label2)
    _, lognorm3, label3 = _estep(X, means, prec, logc, want_resp=False)       # scoring: the sweep runs twice instead
    assert np.array_equal(bits(lognorm), bits(lognorm3)) and np.array_equal(label, label3)
    _, lognorm4, _ = _estep(X, means, prec, logc, want_resp=False, want_label=False)
    assert np.array_equal(bits(lognorm), bits(lognorm4))
    done = _state(1, 3, 1, 0)
    r5, l5, b5 = G(torch.float64, K, N), G(torch.float64, N), G(torch.int32, N)
    call("rbvae_gmm_estep", _dev(X), N, Ld, _dev(means), _dev(prec), _dev(logc), K, r5.t, l5.t, b5.t, done)
    for g, name in ((r5, "resp"), (l5, "lognorm"), (b5, "label")):
        untouched(g, name + " behind done")
    assert done.cpu().tolist() == [1, 3, 1, 0]


def test_estep_far_row():
    """a row 1e3 standard deviations from every mean: lognorm is finite and the responsibilities add to 1"""
    X, means, prec, logc, _, covars = R.params_case(65, 3, 4)
    X[7] = (means.max() + 1e3 * np.sqrt(covars.max())).astype(np.float32)
    ref, resp, lognorm, _ = _check_estep(X, means, prec, logc, "far row")
    assert np.isfinite(lognorm).all() and lognorm[7] < -1e5
    total = float(resp[7].astype(R.LD).sum())
    assert abs(total - 1.0) <= ref["b_r"][7].sum() + 4 * R.U < 1e-6
    with np.errstate(all="ignore"):
        assert not np.isfinite(R.estep(X, means, prec, logc, "lognorm_without_max")[1][7])


def test_estep_exact_ties():
    """two components given twice: every row ties exactly, the label goes to the lower and the responsibilities are equal"""
    X, means, prec, logc, _, _ = R.params_case(300, 5, 2)
    means, prec, logc = np.concatenate([means, means]), np.concatenate([prec, prec]), np.concatenate([logc, logc])
    ref = R.estep_bounds(X, means, prec, logc)
    resp, lognorm, label = _estep(X, means, prec, logc)
    assert np.all(label < 2) and np.array_equal(label, ref["label"])
    assert not np.array_equal(label, R.estep(X, means, prec, logc, "tie_high")[3])
    assert np.array_equal(bits(resp[:, :2].copy()), bits(resp[:, 2:].copy()))
    R.within(resp, ref["resp"], ref["b_r"], "resp of tied components")
    R.within(lognorm, ref["lognorm"], ref["b_ln"], "lognorm of tied components")


def test_estep_variance_of_reg_covar_alone():
    X, means, _, _, w, covars = R.params_case(65, 3, 4)
    means[1], covars[1] = X[5].astype(np.float64), 1e-6     # a component that is one row: s = 1e3
    prec = 1.0 / np.sqrt(covars)
    logc = (np.log(w) + np.log(prec).sum(axis=1)) - 0.5 * 3 * R.LOG_2PI
    ref, resp, lognorm, label = _check_estep(X, means, prec, logc, "variance = reg_covar")
    assert label[5] == 1 and resp[5, 1] > 0.999999 and int((label == 1).sum()) == 1


# ---- M-step ------------------------------------------------------------------------------------------------------------------

def _mstep(X, resp, reg_covar=1e-6, state=None):
    N, Ld = X.shape
    K = resp.shape[1]
    weights, logc = G(torch.float64, K), G(torch.float64, K)
    means, covars, prec = (G(torch.float64, K, Ld) for _ in range(3))
    ws = G(torch.float64, query("rbvae_gmm_ws_bytes", N, Ld, K) // 8)
    call("rbvae_gmm_mstep", _dev(X), N, Ld, _dev(resp.T), K, reg_covar, weights.t, means.t, covars.t, prec.t, logc.t, ws.t,
         state)
    what = f"({N}, {Ld}, {K})"
    got = {n: out(g, f"{n} {what}") for n, g in (("weights", weights), ("means", means), ("covars", covars), ("prec", prec),
                                                  ("logc", logc), ("ws", ws))}
    blocks = R.blocks_rows(N)[0]
    part = got["ws"][:blocks * K * (Ld + 1)].reshape(blocks, K, Ld + 1)[:, :, Ld]
    nk = np.zeros(K)
    for b in range(blocks):                                 # the header's order: the blocks' sums in block order
        nk = nk + part[b]
    got["nk"] = nk + R.NK_EPS
    return got


MSTEP_CASES = [(1, 1, 1, "one_hot"), (300, 7, 5, "soft"), (300, 7, 5, "one_hot"), (300, 7, 5, "empty"), (300, 7, 5, "one"),
               (300, 7, 5, "unnormalised"), (257, 50, 17, "soft"), (300, 128, 17, "soft"), (300, 2, 256, "soft"),
               (65537, 2, 2, "soft")]


@pytest.mark.parametrize("N,Ld,K,kind", MSTEP_CASES)
def test_mstep(N, Ld, K, kind):
    X = R.soft_rows(N, Ld, N + Ld)
    resp = 0.7 * R.resp_case(N, K, "soft") if kind == "unnormalised" else R.resp_case(N, K, kind)
    got = _mstep(X, resp)
    ref = R.mstep_bounds(X, resp, 1e-6, got["means"], got["covars"], got["weights"])
    worst = {n: R.within(got[n], ref[n], ref["b_" + n], f"{n} ({N}, {Ld}, {K}, {kind})")
             for n in ("nk", "means", "covars", "weights", "prec", "logc")}
    total = float(got["weights"].astype(R.LD).sum())
    assert abs(total - 1.0) <= 2 * K * R.U, total           # K ulp
    print(f"M-step ({N}, {Ld}, {K}, {kind}): worst |err|/bound " + ", ".join(f"{n} {v:.3g}" for n, v in worst.items())
          + f"; sum of weights - 1 = {total - 1.0:.3g}")
    if kind == "unnormalised":
        assert R.rejects(R.mstep(X, resp, defect="weights_over_n")[0], ref["weights"], ref["b_weights"])
    if kind == "one_hot":                                   # equal to the per-cluster mean and variance
        lab = resp.argmax(axis=1)
        for k in np.unique(lab):
            rows = X[lab == k].astype(R.LD)
            mu = rows.mean(0)
            var = ((rows - got["means"][k].astype(R.LD)) ** 2).mean(0) + R.LD(1e-6)
            eps = R.NK_EPS / int((lab == k).sum())          # nk = n + 10 eps divides where the plain mean has n
            assert np.all(np.abs(got["means"][k] - mu.astype(np.float64)) <= ref["b_means"][k] + eps * np.abs(got["means"][k]))
            assert np.all(np.abs(got["covars"][k] - var.astype(np.float64)) <= ref["b_covars"][k] + eps * got["covars"][k])
    if kind == "empty":                                     # scikit-learn's formulas as they stand
        k = K // 2
        assert got["nk"][k] == R.NK_EPS and np.all(got["means"][k] == 0.0) and np.all(got["covars"][k] == 1e-6)
        assert 0.0 < got["weights"][k] < 1e-15
    if kind == "one":
        k = K // 2
        assert abs(got["weights"][k] - 1.0) < 1e-15 and np.all(np.delete(got["covars"], k, axis=0) == 1e-6)
    if N == 65537:
        assert R.blocks_rows(N) == (256, 257) and N - 255 * 257 == 2       # all 256 row blocks, the last one ragged
    again = _mstep(X, resp)
    for n in ("weights", "means", "covars", "prec", "logc"):
        assert np.array_equal(bits(got[n]), bits(again[n])), f"two runs differ in {n}"


def test_mstep_behind_done_writes_nothing():
    X, resp = R.soft_rows(300, 7, 1), R.resp_case(300, 5, "soft")
    outs = [G(torch.float64, 5), G(torch.float64, 5, 7), G(torch.float64, 5, 7), G(torch.float64, 5, 7), G(torch.float64, 5),
            G(torch.float64, query("rbvae_gmm_ws_bytes", 300, 7, 5) // 8)]
    done = _state(1, 2, 2, 0)
    call("rbvae_gmm_mstep", _dev(X), 300, 7, _dev(resp.T), 5, 1e-6, outs[0].t, outs[1].t, outs[2].t, outs[3].t, outs[4].t,
         outs[5].t, done)
    for g, name in zip(outs, ("weights", "means", "covars", "prec", "logc", "ws")):
        untouched(g, name + " behind done")
    assert done.cpu().tolist() == [1, 2, 2, 0]


# ---- the decision --------------------------------------------------------------------------------------------------------------

def _decide(lognorm, tol, max_iter, state, prev):
    lb, hist = G(torch.float64, 1), G(torch.float64, max_iter)
    lb.t.fill_(prev)
    hist.t.fill_(-1.0)
    st = G(torch.int32, 4)
    st.t.copy_(_state(*state))
    call("rbvae_gmm_decide", _dev(lognorm), len(lognorm), tol, max_iter, lb.t, hist.t, st.t)
    return out(lb, "lb")[0], out(hist, "history"), out(st, "state").tolist()


@pytest.mark.parametrize("N", [1, 1000, 1025, 70001])
def test_decide_lower_bound(N):
    ln = -9.0 + 11.0 * np.random.RandomState(N).rand(N)
    ref = float(ln.astype(R.LD).sum() / N)
    lb, hist, st = _decide(ln, 0.0, 5, [0, 2, 0, 0], -np.inf)
    w = R.within(np.array([lb]), np.array([ref]), R.lower_bound_bound(ln), f"lower bound of {N} rows")
    print(f"decide, N = {N}: lower bound worst |err|/bound {w:.3g}, equal to the restatement's order: {lb == R.lower_bound(ln)}")
    assert lb == R.lower_bound(ln)                          # the header's order, addition by addition
    assert st == [0, 3, 0, 0] and hist[2] == lb and np.all(np.delete(hist, 2) == -1.0)


def test_decide_outcomes():
    ln = np.full(300, -2.5)                                 # the mean is exactly -2.5
    for prev, tol, max_iter, n_iter, want in ((-2.5 - 0.000999, 1e-3, 9, 4, [1, 5, 1, 0]),     # converged
                                              (-2.5 - 0.001001, 1e-3, 9, 4, [0, 5, 0, 0]),     # running
                                              (-2.5 - 0.001001, 1e-3, 5, 4, [1, 5, 2, 0]),     # max_iter
                                              (-2.5 - 0.000999, 1e-3, 5, 4, [1, 5, 1, 0]),     # both: converged comes first
                                              (-2.5, 0.0, 9, 0, [0, 1, 0, 0]),                 # |change| < 0 never holds
                                              (-np.inf, 1e300, 9, 0, [0, 1, 0, 0])):           # the first iteration
        lb, hist, st = _decide(ln, tol, max_iter, [0, n_iter, 0, 0], prev)
        assert st == want and lb == -2.5 and hist[n_iter] == -2.5, (prev, tol, max_iter, st)
    lb, hist = G(torch.float64, 1), G(torch.float64, 5)
    done = _state(1, 3, 1, 0)
    call("rbvae_gmm_decide", _dev(ln), 300, 1e-3, 5, lb.t, hist.t, done)
    untouched(lb, "lb behind done")
    untouched(hist, "history behind done")
    assert done.cpu().tolist() == [1, 3, 1, 0]


# ---- the whole fit --------------------------------------------------------------------------------------------------------------

def _as_dict(fit, X):
    return {"n_iter": fit.n_iter, "converged": fit.converged, "labels": fit.labels.cpu().numpy(), "lower_bound": fit.lower_bound,
            "lower_bounds": fit.lower_bounds, "score_samples": sfv.gmm_score_samples(fit, X).cpu().numpy(),
            "means": fit.means.cpu().numpy(), "weights": fit.weights.cpu().numpy(), "covars": fit.covariances.cpu().numpy(),
            "bic": sfv.gmm_bic(fit, X), "aic": sfv.gmm_aic(fit, X)}


def _same(a, b):
    return (all(torch.equal(getattr(a, n).view(torch.int64), getattr(b, n).view(torch.int64))
                for n in ("weights", "means", "covariances", "precisions_cholesky", "log_const"))
            and torch.equal(a.labels, b.labels) and a.n_iter == b.n_iter and a.converged == b.converged
            and a.lower_bound == b.lower_bound and np.array_equal(bits(a.lower_bounds), bits(b.lower_bounds)))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("K", KS)
def test_fit_against_sklearn(gold, K, seed):
    t = f"{K}_{seed}"
    fit = sfv.gmm(gold["Xd"], K, init=gold["init_" + t])
    assert fit.labels.dtype == torch.int32 and fit.labels.is_cuda and fit.means.dtype == torch.float64 and fit.means.is_cuda
    assert fit.lower_bounds.dtype == np.float64 and fit.lower_bound == fit.lower_bounds[-1]
    bad, diff = R.against_fixture(_as_dict(fit, gold["Xd"]), gold, t)
    print(f"K = {K}, seed {seed}: device against scikit-learn " + ", ".join(f"{k} {v:.3g}" for k, v in diff.items()))
    assert not bad, (bad, diff)
    assert _same(fit, sfv.gmm(gold["Xd"], K, init=_dev(gold["init_" + t]))), "two runs differ"
    own = sfv.gmm(gold["Xd"], K, seed=seed)                 # from symbols.kmeans' labels
    assert _same(fit, own)
    assert torch.equal(sfv.gmm_predict(fit, gold["Xd"]), fit.labels)
    proba = sfv.gmm_predict_proba(fit, gold["Xd"])
    assert tuple(proba.shape) == (320, K) and torch.equal(proba.argmax(dim=1).int(), fit.labels)
    assert float((proba.sum(dim=1) - 1).abs().max()) <= 1e-12
    ll = sfv.gmm_score_samples(fit, gold["Xd"]).cpu().numpy()
    assert sfv.gmm_score(fit, gold["Xd"]) == R.lower_bound(ll)
    assert abs(sfv.gmm_bic(fit, gold["Xd"]) / R.criteria(R.lower_bound(ll), 320, K, 50)[0] - 1) <= 4 * R.U


def test_fit_short_and_unused(gold):
    fit = sfv.gmm(gold["Xd"], 8, init=gold["init_8_42"], max_iter=3)
    bad, diff = R.against_fixture(_as_dict(fit, gold["Xd"]), gold, "short")
    assert not bad and not fit.converged and fit.n_iter == 3 and len(fit.lower_bounds) == 3, (bad, diff)
    fit = sfv.gmm(gold["Xd"], 4, init=gold["init_unused"])
    bad, diff = R.against_fixture(_as_dict(fit, gold["Xd"]), gold, "unused")
    print("unused component: device against scikit-learn " + ", ".join(f"{k} {v:.3g}" for k, v in diff.items()))
    assert not bad, (bad, diff)
    assert float(fit.weights[2]) < 1e-15 and bool((fit.means[2] == 0).all()) and bool((fit.covariances[2] == 1e-6).all())


@pytest.mark.parametrize("K,seed", [(32, 42), (8, 42), (17, 0)])
def test_run_ahead_changes_nothing(gold, K, seed):
    """iterations are enqueued eight at a time; those behind the decision must leave everything as it was: the fit equals
    one whose max_iter is exactly the iteration it converged at (5: inside the first batch, 8: the last of the first, 15:
    inside the second)"""
    t = f"{K}_{seed}"
    n = int(gold["n_iter_" + t])
    assert n == {32: 5, 8: 8, 17: 15}[K] and sfv.mixture.ENQUEUE == 8
    fit = sfv.gmm(gold["Xd"], K, init=gold["init_" + t])
    exact = sfv.gmm(gold["Xd"], K, init=gold["init_" + t], max_iter=n)
    assert exact.converged and exact.n_iter == n and _same(fit, exact)
    before = sfv.gmm(gold["Xd"], K, init=gold["init_" + t], max_iter=n - 1)
    assert not before.converged and before.n_iter == n - 1
    assert np.array_equal(bits(before.lower_bounds), bits(fit.lower_bounds[:n - 1]))


@pytest.mark.parametrize("seed", SEEDS)
def test_select(gold, seed):
    for criterion, want in (("bic", 2), ("aic", 8)):
        table, K, fit = sfv.gmm_select(gold["Xd"], KS, criterion=criterion, seed=seed)
        assert K == want and fit.means.shape[0] == want and [row["K"] for row in table] == list(KS)
        for row in table:
            t = f"{row['K']}_{seed}"
            assert row["n_iter"] == int(gold["n_iter_" + t]) and row["converged"]
            assert abs(row["bic"] / float(gold["bic_" + t]) - 1) <= 1e-10 and abs(row["aic"] / float(gold["aic_" + t]) - 1) <= 1e-10
            assert abs(row["score"] - float(gold["score_samples_" + t].mean())) <= 1e-10
        assert _same(fit, sfv.gmm(gold["Xd"], want, seed=seed))


def test_latent_mixture():
    F_, RES, LD = 40, 64, 16
    torch.manual_seed(0)
    model = sfv.Seq2SeqBinaryVAE(3, 3, LD, LD, variant="contrastive", input_hw=(RES, RES), compute_dtype="f32").cuda().eval()
    x = torch.rand(F_, 3, RES, RES, generator=torch.Generator().manual_seed(1)).cuda()
    u = torch.rand(F_, LD, generator=torch.Generator().manual_seed(2))
    flags = [10, 30]
    res = sfv.latent_mixture(model, x, range(F_), flags, u=u, ks=(2, 3, 4))
    sym = sfv.latent_symbols(model, x, range(F_), flags, u=u)
    assert torch.equal(res["latents"], sym["latents"]) and np.array_equal(res["labels"], sym["labels"]) and not model.training
    fit = res["gmm"]
    assert fit.means.shape == (3, LD) and _same(fit, sfv.gmm(res["latents"], 3))
    ref = sfv.clustering_agreement(res["labels"], fit.labels, 3, 3)
    assert all(res["agreement"][n] == ref[n] and np.isfinite(ref[n]) for n in ("ari", "nmi", "v_measure", "fowlkes_mallows"))
    proba = sfv.gmm_predict_proba(fit, res["latents"])
    assert torch.equal(res["responsibilities"], proba)
    assert res["mean_max_responsibility"] == float(proba.max(dim=1).values.mean()) and 1 / 3 <= res["mean_max_responsibility"] <= 1
    assert torch.equal(res["log_likelihood"], sfv.gmm_score_samples(fit, res["latents"]))
    assert torch.equal(res["entropy"], torch.special.entr(proba).sum(dim=1))
    assert float(res["entropy"].min()) >= 0.0 and float(res["entropy"].max()) <= np.log(3) + 1e-12
    table, K, best = res["selection"]
    t2, K2, b2 = sfv.gmm_select(res["latents"], (2, 3, 4))
    assert table == t2 and K == K2 and _same(best, b2)
    proj = {"latents": res["latents"].clone()}
    again = sfv.latent_mixture(model, x, range(F_), flags, projections=proj, n_components=4)
    assert again["gmm"].means.shape == (4, LD) and again["agreement"]["contingency"].shape == (3, 4) and "selection" not in again


# ---- refused arguments --------------------------------------------------------------------------------------------------------------

def test_refused_arguments_write_nothing():
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")       # noqa: E731
    zd = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")      # noqa: E731
    resp, lognorm, label, state = G(torch.float64, 64), G(torch.float64, 8), G(torch.int32, 8), G(torch.int32, 4)
    weights, logc = G(torch.float64, 257), G(torch.float64, 257)
    means, covars, prec = (G(torch.float64, 257, 129) for _ in range(3))
    ws, lb, hist = G(torch.float64, 4096), G(torch.float64, 1), G(torch.float64, 4)
    X, par, vec = z(300, 129), zd(257, 129), zd(300)
    big = (1 << 18) + 1                                     # N K = 2^26 + 256: over the cap, every pointer is refused unread
    for N, Ld, K, match in ((8, 3, 9, "K=9"), (8, 129, 2, "L=129"), (300, 3, 257, "K=257"), (0, 3, 1, "N=0"),
                            ((1 << 20) + 1, 3, 2, "N=1048577"), (8, 0, 2, "L=0"), (8, 3, 0, "K=0"), (big, 2, 256, f"N={big}")):
        assert query("rbvae_gmm_ok", N, Ld, K) == 0 and query("rbvae_gmm_ws_bytes", N, Ld, K) == 0
        with pytest.raises(RuntimeError, match=match):
            call("rbvae_gmm_estep", X, N, Ld, par, par, vec, K, resp.t, lognorm.t, label.t, state.t)
        with pytest.raises(RuntimeError, match=match):
            call("rbvae_gmm_mstep", X, N, Ld, vec, K, 1e-6, weights.t, means.t, covars.t, prec.t, logc.t, ws.t, None)
    for N, match in ((0, "N=0"), ((1 << 20) + 1, "N=1048577")):
        with pytest.raises(RuntimeError, match=match):
            call("rbvae_gmm_decide", vec, N, 1e-3, 4, lb.t, hist.t, state.t)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_gmm_estep", X, 8, 3, None, par, vec, 2, resp.t, lognorm.t, label.t, state.t)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_gmm_mstep", X, 8, 3, vec, 2, 1e-6, weights.t, means.t, covars.t, prec.t, logc.t, None, None)
    with pytest.raises(ValueError, match="reg_covar"):
        call("rbvae_gmm_mstep", X, 8, 3, vec, 2, -1e-6, weights.t, means.t, covars.t, prec.t, logc.t, ws.t, None)
    with pytest.raises(ValueError, match="max_iter=0"):
        call("rbvae_gmm_decide", vec, 8, 1e-3, 0, lb.t, hist.t, state.t)
    with pytest.raises(ValueError, match="tol"):
        call("rbvae_gmm_decide", vec, 8, -1.0, 4, lb.t, hist.t, state.t)
    for g, what in ((resp, "resp"), (lognorm, "lognorm"), (label, "label"), (state, "state"), (weights, "weights"), (logc, "logc"),
                    (means, "means"), (covars, "covars"), (prec, "prec_chol"), (ws, "workspace"), (lb, "lb"), (hist, "history")):
        untouched(g, what)
    bad = z(8, 3)
    bad[2, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        sfv.gmm(bad, 2)
    ok = torch.rand(8, 3, generator=torch.Generator().manual_seed(0)).cuda()
    fit = sfv.gmm(ok, 2, init=np.array([0, 0, 0, 0, 1, 1, 1, 1]))
    for fn, match in ((lambda: sfv.gmm(z(8, 3), 9), "K=9"), (lambda: sfv.gmm(z(8, 129), 2), "L=129"),
                      (lambda: sfv.gmm(z(300, 3), 257), "K=257"), (lambda: sfv.gmm(z(8, 3).cpu(), 2), "GPU"),
                      (lambda: sfv.gmm(z(8, 3).double(), 2), "float32"), (lambda: sfv.gmm(z(8, 3), 2, max_iter=0), "max_iter"),
                      (lambda: sfv.gmm(z(8, 3), 2, tol=-1.0), "tol"), (lambda: sfv.gmm(z(8, 3), 2, reg_covar=-1.0), "reg_covar"),
                      (lambda: sfv.gmm(z(8, 3), 2, init="random"), "init"),
                      (lambda: sfv.gmm(z(8, 3), 2, init=np.array([0, 0, 0, 0, 1, 1, 1, 2])), "labels in"),
                      (lambda: sfv.gmm(z(8, 3), 2, init=np.array([0, 0, 0, -1, 1, 1, 1, 1])), "labels in"),
                      (lambda: sfv.gmm(z(8, 3), 2, init=np.array([0, 1, 1])), "labels in"),
                      (lambda: sfv.gmm(z(8, 3), 2, init=np.zeros(8)), "integers"),
                      (lambda: sfv.gmm(torch.empty((big, 2), dtype=torch.float32, device="cuda"), 256), f"N={big}"),
                      (lambda: sfv.gmm_predict(fit, z(8, 4)), "columns"), (lambda: sfv.gmm_score_samples(fit, ok.cpu()), "GPU"),
                      (lambda: sfv.gmm_predict_proba(fit, bad), "NaN"), (lambda: sfv.gmm_select(ok, [2], criterion="icl"), "criterion"),
                      (lambda: sfv.latent_mixture(None, z(2, 3, 8, 8), [0], [1]), "frame indices")):
        with pytest.raises(ValueError, match=match):
            fn()
