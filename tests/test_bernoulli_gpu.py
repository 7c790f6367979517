"""GPU: the kernels of the Bernoulli models of the hard codes (csrc/bernoulli.hip) inside sentinel guard bands (tests/_bounds.py's
buffers) against tests/_bernoulli_ref.py -- the packed words, logb, rowmax, the M-step's block partials, S, nk, theta and the
weights bit for bit against the f64 restatement (selections, additions in one order and IEEE quotients), e, resp, lognorm and
the three log tables inside the long double bounds -- and bernoulli.py end to end against the restatement's fits at the measured
gates of tests/test_bernoulli_cpu.py (64 times the f64 / long double difference of each quantity).

lp is held in resp only until resp is written, so its bits are seen through logb (the same sum without log w), through the
labels (equal to the restatement's on every row) and at K = 1, where lognorm = lp exactly.  rbvae_hmm_ok refuses K > 64, so
(300, 33, 65) runs the E-step only and asserts that the emissions are refused.  Every test prints its worst |error| / bound;
DESIGN.md section 7 quotes them.

Measured on one MI355X: every bit-for-bit comparison holds; e is at most 0.37 of its bound (300 x 2 x 64), lognorm 0.061, resp
0.144, log theta 0.37, log(1 - theta) 0.30, log w 0.  On the planted chains and the fixture's codes n_iter, converged / why, every
label and every row of the path equal the restatement's and every quantity is at least 16 times inside its gate; bmm_select
picks K = 5 of (3, 5, 7) as the restatement does.  The 26 tests take about 5 s together.
"""
import functools

import numpy as np
import pytest
import torch

import _bounds as B
import _gmm_ref as Gm
import _hmm_ref as H
import _bernoulli_ref as R
import sfv_amd as sfv

pytestmark = pytest.mark.gpu

GUARD = 4096
B.SENTINEL.setdefault(torch.float64, (torch.int64, 0x7FF8DEADDEADBEEF))
B.SENTINEL.setdefault(torch.int32, (torch.int32, -0x21524111))
call, query = sfv._lib.call, sfv._lib.query
F64, I32 = torch.float64, torch.int32


def G(dtype, *shape):
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


def _bits(X):
    """the restatement's packed words on the device, as the int32 the package holds"""
    return _dev(R.pack(X).view(np.int32))


def _state(*v):
    return torch.tensor(list(v) or [0, 0, 0, 0], dtype=torch.int32, device="cuda")


def bits(a):
    return np.asarray(a).view(np.int64) if np.asarray(a).dtype == np.float64 else np.asarray(a)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- pack --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [1, 31, 32, 33, 64, 65, 127, 128])
def test_pack(L):
    for N in (2, 63, 64, 65, 257):
        X = R.tables_case(N, L, 1)[0]
        if 0 < N // 2 < N - 1:
            X[N // 2, L // 2] = np.nan                      # not > 0.5
        X[0, 0], X[N - 1, L - 1] = 0.5, np.nextafter(np.float32(0.5), np.float32(1))        # not set; set
        g = G(I32, N, 4)
        call("rbvae_bern_pack", _dev(X), N, L, g.t)
        got = out(g, f"bits ({N}, {L})").view(np.uint32)
        want = R.pack(X)
        assert np.array_equal(got, want), f"({N}, {L})"
        if L < 128:                                         # the padding bits are zero
            full = np.unpackbits(got.view(np.uint8), bitorder="little").reshape(N, 128)
            assert not full[:, L:].any() and np.array_equal(full[:, :L].astype(bool), R.as_bits(X))
        clean = np.nan_to_num(X)                            # the package refuses NaN before the kernel sees it
        assert torch.equal(sfv.pack_codes(_dev(clean)).cpu(), torch.from_numpy(R.pack(clean).view(np.int32)))
        if np.isnan(X).any():
            with pytest.raises(ValueError, match="NaN"):
                sfv.pack_codes(_dev(X))


# ---- emissions and the E-step ------------------------------------------------------------------------------------------------

def _emit(X, logt, logf, state=None, want=True):
    N, L = X.shape
    K = len(logt)
    logb, rowmax, e = G(F64, K, N), G(F64, N), G(F64, N, K)
    call("rbvae_bern_emit", _bits(X), N, L, _dev(logt), _dev(logf), K, logb.t, rowmax.t, e.t, state)
    what = f"({N}, {L}, {K})"
    if not want:
        for g, n in ((logb, "logb"), (rowmax, "rowmax"), (e, "e")):
            untouched(g, n + " behind done " + what)
        return None
    return out(logb, "logb " + what).T, out(rowmax, "rowmax " + what), out(e, "e " + what)


def _estep(X, logt, logf, logw, state=None, resp=True, label=True, want=True):
    N, L = X.shape
    K = len(logt)
    r, ln, lab = (G(F64, K, N) if resp else None), G(F64, N), (G(I32, N) if label else None)
    call("rbvae_bern_estep", _bits(X), N, L, _dev(logt), _dev(logf), _dev(logw), K, r.t if resp else None, ln.t,
         lab.t if label else None, state)
    what = f"({N}, {L}, {K})"
    if not want:
        for g, n in ((r, "resp"), (ln, "lognorm"), (lab, "label")):
            if g is not None:
                untouched(g, n + " behind done " + what)
        return None
    return (out(r, "resp " + what).T if resp else None, out(ln, "lognorm " + what), out(lab, "label " + what) if label else None)


SHAPES = [(2, 1, 1), (257, 128, 17), (300, 2, 64), (300, 33, 65), (300, 100, 41)]


@pytest.mark.parametrize("N,L,K", SHAPES)
def test_emit_and_estep(N, L, K):
    X, logt, logf, logw = R.tables_case(N, L, K)
    what = f"({N}, {L}, {K})"
    w = []
    if (N, L, K) == (257, 128, 17):
        assert K > query("rbvae_bern_chunk_components", L) == 16        # more than one LDS chunk, the last of one component
    if (N, L, K) == (300, 100, 41):
        assert query("rbvae_bern_chunk_components", L) == 20            # three chunks: 20, 20 and 1
    if H.ok(N, L, K):
        ref = R.emit_bounds(X, logt, logf)
        lb_r, m_r, e_r = R.emit(X, logt, logf)
        lb, m, e = _emit(X, logt, logf)
        assert same(lb, lb_r) and same(m, m_r), "logb and rowmax are selections and additions in one order"
        assert (e.max(axis=1) == 1.0).all()
        w.append(R.within(e, ref["e"], ref["b_e"], "e " + what))
        again = _emit(X, logt, logf, _state())
        assert all(same(a, b) for a, b in zip((lb, m, e), again)), "two runs differ"
        _emit(X, logt, logf, _state(1, 3, 1, 0), want=False)
    else:
        assert query("rbvae_bern_ok", N, L, K) == 1 and query("rbvae_hmm_ok", N, L, K) == 0
        gs = [G(F64, K, N), G(F64, N), G(F64, N, K)]
        with pytest.raises(RuntimeError, match="rbvae_hmm_ok"):
            call("rbvae_bern_emit", _bits(X), N, L, _dev(logt), _dev(logf), K, gs[0].t, gs[1].t, gs[2].t, None)
        for g in gs:
            untouched(g, "an output of refused emissions")
    er = R.estep_bounds(X, logt, logf, logw)
    lp_r, ln_r, resp_r, label_r = R.estep(X, logt, logf, logw)
    resp, ln, label = _estep(X, logt, logf, logw)
    w += [R.within(ln, er["lognorm"], er["b_ln"], "lognorm " + what), R.within(resp, er["resp"], er["b_r"], "resp " + what)]
    assert np.array_equal(label, label_r), "lp is the restatement's bit for bit, so every label is"
    assert np.array_equal(label[er["decided"]], er["label"][er["decided"]])
    if K == 1:
        assert same(ln, lp_r[:, 0]) and (resp == 1.0).all()  # lognorm = lp + log 1
    _, ln2, lab2 = _estep(X, logt, logf, logw, resp=False)   # the two-sweep form
    _, ln3, _ = _estep(X, logt, logf, logw, _state(), resp=False, label=False)
    resp4, ln4, _ = _estep(X, logt, logf, logw, label=False)
    assert same(ln, ln2) and same(ln, ln3) and same(ln, ln4) and same(resp, resp4) and np.array_equal(label, lab2)
    _estep(X, logt, logf, logw, _state(1, 3, 1, 0), want=False)
    print(f"emit / E-step {what}: logb, rowmax and the labels equal the restatement's; worst |err|/bound "
          f"{'e, ' if len(w) == 3 else ''}lognorm, resp = " + ", ".join(f"{x:.3g}" for x in w))


# ---- M-step ------------------------------------------------------------------------------------------------------------------

def _mstep(X, resp, prior, state=None, want=True):
    N, L = X.shape
    K = resp.shape[1]
    n = query("rbvae_bern_ws_bytes", N, L, K)
    assert n == R.ws_bytes(N, L, K)
    blocks = Gm.blocks_rows(N)[0]
    gs = {"weights": G(F64, K), "logw": G(F64, K), "theta": G(F64, K, L), "logt": G(F64, K, L), "logf": G(F64, K, L),
          "ws": G(F64, blocks, K, L + 1)}
    call("rbvae_bern_mstep", _bits(X), N, L, _dev(np.ascontiguousarray(resp.T)), K, prior, gs["weights"].t, gs["logw"].t,
         gs["theta"].t, gs["logt"].t, gs["logf"].t, gs["ws"].t, state)
    what = f"({N}, {L}, {K})"
    if not want:
        for name, g in gs.items():
            untouched(g, name + " behind done " + what)
        return None
    return {name: out(g, name + " " + what) for name, g in gs.items()}


def _posterior_rows():
    """resp rows from a real posterior: the E-step of the fixture's codes under the M-step of their k-means start"""
    X, s, start, K = R.case("fixture")
    M = R.mstep(X, Gm.one_hot(start, K), 1.0)
    return X, R.estep(X, M["logt"], M["logf"], M["logw"])[2]


@pytest.mark.parametrize("case", ["tiny", "soft", "empty", "one_hot", "blocks_256", "posterior"])
def test_mstep(case):
    if case == "posterior":
        X, resp = _posterior_rows()
    else:
        N, L, K, kind = {"tiny": (2, 1, 1, "soft"), "soft": (300, 33, 5, "soft"), "empty": (300, 128, 7, "empty"),
                         "one_hot": (1025, 65, 3, "one_hot"), "blocks_256": (65537, 7, 3, "soft")}[case]
        X, resp = R.tables_case(N, L, K)[0], Gm.resp_case(N, K, kind)
    N, L = X.shape
    K = resp.shape[1]
    prior = 0.75
    got = _mstep(X, resp, prior)
    parts = R.block_partials(X, resp)
    assert same(got["ws"], parts), "every cell's partial: one order of additions"
    S, nk = R.block_totals(got["ws"])
    want = R.mstep(X, resp, prior)
    assert same(S, want["S"]) and same(nk, want["nk"])
    assert same(got["theta"], want["theta"]) and same(got["weights"], want["weights"]), "IEEE quotients of equal sums"
    ref = R.mstep_bounds(X, resp, prior, {"S": S, "nk": nk, "theta": got["theta"], "weights": got["weights"]})
    w = [R.within(got[n], ref[n], ref["b_" + n], f"{n} {case}") for n in ("logt", "logf", "logw")]
    w += [R.within(got["theta"], ref["theta"], ref["b_theta"], "theta"), R.within(got["weights"], ref["weights"], ref["b_weights"], "weights")]
    print(f"M-step {case} ({N}, {L}, {K}): partials, S, nk, theta and weights equal the restatement's; worst |err|/bound logt, logf, "
          f"logw, theta, weights (long double) = " + ", ".join(f"{x:.3g}" for x in w))
    if case == "empty":
        assert np.all(got["theta"][K // 2] == 0.5) and np.all(got["logt"][K // 2] == got["logf"][K // 2])
    if case == "blocks_256":
        assert Gm.blocks_rows(N) == (256, 257)              # all 256 row blocks, the last one ragged
    again = _mstep(X, resp, prior, _state())
    assert all(same(got[n], again[n]) for n in got), "two runs differ"
    _mstep(X, resp, prior, _state(1, 2, 1, 0), want=False)


# ---- refused arguments -------------------------------------------------------------------------------------------------------

def test_refused_arguments_write_nothing():
    zd = lambda *s: torch.zeros(s, dtype=F64, device="cuda")      # noqa: E731
    outs = {n: G(F64, 4096) for n in ("a", "b", "c", "d", "e", "ws")}
    lab, packed = G(I32, 4096), G(I32, 4096)
    X = torch.zeros((300, 129), dtype=torch.float32, device="cuda")
    words = torch.zeros((300, 4), dtype=I32, device="cuda")
    par, mat, vec = zd(257, 129), zd(300, 257), zd(300)
    o = outs
    for N, L, K, match in ((8, 3, 9, "K=9"), (8, 129, 2, "L=129"), (300, 3, 257, "K=257"), (8, 0, 2, "L=0"), (8, 3, 0, "K=0"),
                           ((1 << 20) + 1, 3, 2, "N=1048577"), (1 << 20, 3, 65, "K=65")):
        assert query("rbvae_bern_ok", N, L, K) == 0 and query("rbvae_bern_ws_bytes", N, L, K) == 0
        with pytest.raises(RuntimeError, match=match):
            call("rbvae_bern_emit", words, N, L, par, par, K, o["a"].t, o["b"].t, o["c"].t, None)
        with pytest.raises(RuntimeError, match=match):
            call("rbvae_bern_estep", words, N, L, par, par, vec, K, o["a"].t, o["b"].t, lab.t, None)
        with pytest.raises(RuntimeError, match=match):
            call("rbvae_bern_mstep", words, N, L, mat, K, 1.0, o["a"].t, o["b"].t, o["c"].t, o["d"].t, o["e"].t, o["ws"].t, None)
        if K == 2:
            with pytest.raises(RuntimeError, match=match):
                call("rbvae_bern_pack", X, N, L, packed.t)
    for N, K in ((1, 1), (300, 65)):                        # inside rbvae_bern_ok, outside rbvae_hmm_ok
        assert query("rbvae_bern_ok", N, 3, K) == 1
        with pytest.raises(RuntimeError, match="rbvae_hmm_ok"):
            call("rbvae_bern_emit", words, N, 3, par, par, K, o["a"].t, o["b"].t, o["c"].t, None)
    for prior in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="prior"):
            call("rbvae_bern_mstep", words, 8, 3, mat, 2, prior, o["a"].t, o["b"].t, o["c"].t, o["d"].t, o["e"].t, o["ws"].t, None)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_bern_pack", None, 8, 3, packed.t)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_bern_pack", X, 8, 3, None)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_bern_emit", words, 8, 3, par, None, 2, o["a"].t, o["b"].t, o["c"].t, None)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_bern_emit", words, 8, 3, par, par, 2, o["a"].t, None, o["c"].t, None)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_bern_estep", words, 8, 3, par, par, None, 2, o["a"].t, o["b"].t, lab.t, None)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_bern_estep", words, 8, 3, par, par, vec, 2, o["a"].t, None, lab.t, None)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_bern_mstep", None, 8, 3, mat, 2, 1.0, o["a"].t, o["b"].t, o["c"].t, o["d"].t, o["e"].t, o["ws"].t, None)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_bern_mstep", words, 8, 3, mat, 2, 1.0, o["a"].t, o["b"].t, o["c"].t, o["d"].t, o["e"].t, None, None)
    for n, g in outs.items():
        untouched(g, n)
    untouched(lab, "label")
    untouched(packed, "bits")
    ok = (torch.rand(8, 3, generator=torch.Generator().manual_seed(0)) < 0.5).float().cuda()
    bad = ok.clone()
    bad[2, 1] = float("nan")
    init = np.array([0, 0, 0, 0, 1, 1, 1, 1])
    mix, chain = sfv.bmm(ok, 2, init=init), sfv.bhmm(ok, 2, init=init)
    for fn, match in ((lambda: sfv.bmm(ok.double(), 2), "float32"), (lambda: sfv.bmm(bad, 2), "NaN"), (lambda: sfv.bhmm(bad, 2), "NaN"),
                      (lambda: sfv.bmm(ok, 2, init=np.array([0, 0, 0, 0, 1, 1, 1, 2])), "labels in"),
                      (lambda: sfv.bhmm(ok, 2, init=np.array([0, 1, 1])), "labels in"), (lambda: sfv.bhmm(ok, 2, block_rows=0), "block_rows"),
                      (lambda: sfv.bmm_predict(mix, ok[:, :2].contiguous()), "columns"), (lambda: sfv.bmm_score(mix, ok.cpu()), "GPU"),
                      (lambda: sfv.bhmm_predict(chain, ok[:, :2].contiguous()), "columns"), (lambda: sfv.bhmm_predict_proba(chain, bad), "NaN"),
                      (lambda: sfv.bmm_select(ok, [2], criterion="icl"), "criterion"), (lambda: sfv.bmm(ok, 2, prior=0.0), "prior"),
                      (lambda: sfv.latent_code_models(None, torch.zeros((2, 3, 8, 8), device="cuda"), [0], [1]), "frame indices")):
        with pytest.raises(ValueError, match=match):
            fn()


# ---- whole fits ----------------------------------------------------------------------------------------------------------------

def _mix_dict(fit, Xd):
    return {"weights": fit.weights.cpu().numpy(), "probs": fit.probs.cpu().numpy(), "lower_bounds": fit.lower_bounds,
            "resp": sfv.bmm_predict_proba(fit, Xd).cpu().numpy(), "n_iter": fit.n_iter, "converged": fit.converged,
            "labels": fit.labels.cpu().numpy()}


def _chain_dict(fit):
    return {"pi": fit.startprob.cpu().numpy(), "A": fit.transmat.cpu().numpy(), "probs": fit.probs.cpu().numpy(),
            "log_likelihoods": fit.log_likelihoods, "gamma": fit.posterior.cpu().numpy(), "n_iter": fit.n_iter,
            "converged": fit.converged, "path": fit.path.cpu().numpy()}


def _same_fit(a, b, names):
    return all((torch.equal(x.contiguous().view(torch.int64) if x.dtype == F64 else x, y.contiguous().view(torch.int64) if y.dtype == F64 else y)
                if isinstance(x, torch.Tensor) else (same(x, y) if isinstance(x, np.ndarray) else x == y))
               for x, y in ((getattr(a, n), getattr(b, n)) for n in names))


MIX_FIELDS = ("weights", "probs", "log_probs", "log_1m_probs", "log_weights", "n_iter", "converged", "lower_bound", "lower_bounds", "labels")
CHAIN_FIELDS = ("startprob", "transmat", "probs", "log_probs", "log_1m_probs", "n_iter", "converged", "why", "log_likelihood",
                "log_likelihoods", "posterior", "path", "path_score")


@functools.lru_cache(maxsize=None)
def _device_fits(name):
    X, s, start, K = R.case(name)
    Xd = _dev(X)
    return Xd, sfv.bmm(Xd, K, init=start), sfv.bhmm(Xd, K, init=start)


def _report(what, diff, gates, quantities):
    print(f"{what}: device against the f64 restatement (gate = 64 x f64 / long double difference): "
          + ", ".join(f"{q} {diff[q]:.3g} ({R.GATE_FACTOR * gates[q]:.3g})" for q in quantities))


@pytest.mark.parametrize("name", sorted(R.PLANTED) + ["fixture"])
def test_fits(name):
    X, s, start, K = R.case(name)
    N, L = X.shape
    Xd, mix, chain = _device_fits(name)
    f_mix, _, g_mix = R.fitted(name, "bmm")
    f_chain, _, g_chain = R.fitted(name, "bhmm")
    d = R.differences(_mix_dict(mix, Xd), f_mix, R.BMM_QUANTITIES, "labels")
    _report(f"{name} mixture, n_iter {mix.n_iter} = {f_mix['n_iter']}", d, g_mix, R.BMM_QUANTITIES)
    bad = R.outside(d, g_mix, R.BMM_QUANTITIES, "labels")
    assert not bad, (bad, d)
    assert mix.lower_bound == mix.lower_bounds[-1] and len(mix.lower_bounds) == mix.n_iter and mix.labels.dtype == I32
    d = R.differences(_chain_dict(chain), f_chain, R.BHMM_QUANTITIES, "path")
    _report(f"{name} hidden Markov model, n_iter {chain.n_iter} = {f_chain['n_iter']}", d, g_chain, R.BHMM_QUANTITIES)
    bad = R.outside(d, g_chain, R.BHMM_QUANTITIES, "path")
    assert not bad, (bad, d)
    assert chain.why == f_chain["why"] and chain.log_likelihood == chain.log_likelihoods[-1] and len(chain.log_likelihoods) == chain.n_iter
    assert chain.path.dtype == I32 and tuple(chain.posterior.shape) == (N, K) and tuple(chain.probs.shape) == (K, L)
    a0, a1, a2 = H.ari(s, start), H.ari(s, mix.labels.cpu().numpy()), H.ari(s, chain.path.cpu().numpy())
    print(f"{name}: ARI of the k-means start {a0:.3f}, of the mixture's labels {a1:.3f}, of the device's Viterbi path {a2:.3f}")
    assert a2 >= 0.85 and a2 >= a0
    # prediction and scoring with the fits' own parameters
    assert torch.equal(sfv.bmm_predict(mix, Xd), mix.labels) and torch.equal(sfv.bhmm_predict(chain, Xd), chain.path)
    assert torch.equal(sfv.bhmm_predict_proba(chain, Xd), chain.posterior)
    ln = sfv.bmm_score_samples(mix, Xd).cpu().numpy()
    ll = sfv.bhmm_score_samples(chain, Xd).cpu().numpy()
    assert sfv.bmm_score(mix, Xd) == Gm.lower_bound(ln) and sfv.bhmm_score(chain, Xd) == Gm.lower_bound(ll)
    assert abs(sfv.bmm_score(mix, Xd) - f_mix["score"]) <= R.GATE_FACTOR * g_mix["lower_bounds"]
    assert abs(sfv.bhmm_score(chain, Xd) - f_chain["score"]) <= R.GATE_FACTOR * g_chain["log_likelihoods"]
    for got, score, p in ((sfv.bmm_bic(mix, Xd), Gm.lower_bound(ln), R.bmm_n_parameters(K, L)),
                          (sfv.bhmm_bic(chain, Xd), Gm.lower_bound(ll), R.bhmm_n_parameters(K, L))):
        assert abs(got / R.criteria(score, N, p)[0] - 1) <= 4 * R.U
    assert abs(sfv.bmm_aic(mix, Xd) / R.criteria(Gm.lower_bound(ln), N, K * L + K - 1)[1] - 1) <= 4 * R.U
    assert abs(sfv.bhmm_aic(chain, Xd) / R.criteria(Gm.lower_bound(ll), N, (K - 1) + K * (K - 1) + K * L)[1] - 1) <= 4 * R.U
    assert abs(sfv.bmm_bic(mix, Xd) / R.criteria(Gm.lower_bound(ln), N, Gm.n_parameters(K, L))[0] - 1) > 1e-3     # not the Gaussian count
    # two runs agree bit for bit; the tables are the logs of the probabilities
    assert _same_fit(mix, sfv.bmm(Xd, K, init=_dev(start)), MIX_FIELDS) and _same_fit(chain, sfv.bhmm(Xd, K, init=_dev(start)), CHAIN_FIELDS)
    th = chain.probs.cpu().numpy()
    assert np.abs(chain.log_probs.cpu().numpy() - np.log(th)).max() <= 1e-14 and (th > 0).all() and (th < 1).all()


def test_default_start_and_run_ahead():
    """init="kmeans" is symbols.kmeans' labelling of the codes; iterations enqueued behind the decision leave everything as it
    was: the fit equals one whose max_iter is exactly the iteration it converged at (10: the second of the second batch)"""
    X, s, start, K = R.case("nine_states")
    Xd, mix, chain = _device_fits("nine_states")
    own = sfv.kmeans(Xd, K, seed=42).labels
    assert _same_fit(sfv.bmm(Xd, K), sfv.bmm(Xd, K, init=own), MIX_FIELDS)
    assert _same_fit(sfv.bhmm(Xd, K, max_iter=3), sfv.bhmm(Xd, K, init=own, max_iter=3), CHAIN_FIELDS)
    n = chain.n_iter
    assert n == R.fitted("nine_states", "bhmm")[0]["n_iter"] == 10 and sfv.bernoulli.ENQUEUE == 8
    exact = sfv.bhmm(Xd, K, init=start, max_iter=n)
    assert exact.converged and _same_fit(chain, exact, CHAIN_FIELDS)
    before = sfv.bhmm(Xd, K, init=start, max_iter=n - 1)
    assert not before.converged and before.why == "max_iter" and before.n_iter == n - 1
    assert same(before.log_likelihoods, chain.log_likelihoods[:n - 1])
    m = mix.n_iter
    exact = sfv.bmm(Xd, K, init=start, max_iter=m)
    assert exact.converged and _same_fit(mix, exact, MIX_FIELDS)
    other = sfv.bhmm(Xd, K, init=start, block_rows=900)     # the plain recursion: another order, the same decisions
    g = R.fitted("nine_states", "bhmm")
    assert other.n_iter == n and not R.outside(R.differences(_chain_dict(other), g[0], R.BHMM_QUANTITIES, "path"), g[2],
                                               R.BHMM_QUANTITIES, "path")


def test_select_picks_the_restatements_k():
    X, s, _, _ = R.case("fixture")
    Xd = _dev(X)
    ks = (3, 5, 7)
    bic = []
    for K in ks:
        start = H.kmeans_labels(X, K, 42)
        bic.append(R.bmm_fit(X, start, K)["bic"])
    table, K, best = sfv.bmm_select(Xd, ks)
    print("bmm_select: BIC of the restatement " + ", ".join(f"{b:.2f}" for b in bic) + "; of the device "
          + ", ".join(f"{row['bic']:.2f}" for row in table) + f"; chosen K = {K}")
    assert [row["K"] for row in table] == list(ks) and K == R.FIXTURE[2] == Gm.choose(ks, bic)
    for row in table:
        fit = sfv.bmm(Xd, row["K"])
        assert row["n_iter"] == fit.n_iter and row["converged"] == fit.converged and row["score"] == sfv.bmm_score(fit, Xd)
        assert row["bic"] == sfv.bmm_bic(fit, Xd) and row["aic"] == sfv.bmm_aic(fit, Xd)
        if row["K"] == K:
            assert _same_fit(best, fit, MIX_FIELDS)
    table2, K2, best2 = sfv.bhmm_select(Xd, (4, 5), max_iter=6)
    assert [row["K"] for row in table2] == [4, 5] and K2 in (4, 5) and best2.probs.shape[0] == K2
    assert table2[1]["bic"] == sfv.bhmm_bic(sfv.bhmm(Xd, 5, max_iter=6), Xd)


def test_latent_code_models_agrees_with_its_parts():
    F_, RES, LD = 40, 64, 16
    torch.manual_seed(0)
    model = sfv.Seq2SeqBinaryVAE(3, 3, LD, LD, variant="contrastive", input_hw=(RES, RES), compute_dtype="f32").cuda().eval()
    x = torch.rand(F_, 3, RES, RES, generator=torch.Generator().manual_seed(1)).cuda()
    u = torch.rand(F_, LD, generator=torch.Generator().manual_seed(2))
    flags = [10, 30]
    res = sfv.latent_code_models(model, x, range(F_), flags, u=u, ks=(2, 3))
    assert set(res) == {"codes", "labels", "bmm", "bhmm", "bmm_agreement", "bhmm_agreement", "kmeans_agreement", "prototypes",
                        "bit_reliability", "change_points", "boundaries", "dwell", "selection"}
    codes = res["codes"]
    assert tuple(codes.shape) == (F_, LD) and codes.dtype == torch.float32 and bool(torch.isfinite(codes).all())
    assert np.array_equal(res["labels"], sfv.latent_hmm(model, x, range(F_), flags, u=u)["labels"]) and not model.training
    start = sfv.kmeans(codes, 3, seed=42).labels
    mix, chain = res["bmm"], res["bhmm"]
    assert _same_fit(mix, sfv.bmm(codes, 3, init=start), MIX_FIELDS) and _same_fit(chain, sfv.bhmm(codes, 3, init=start), CHAIN_FIELDS)
    for key, lab in (("bmm_agreement", mix.labels), ("bhmm_agreement", chain.path), ("kmeans_agreement", start)):
        ref = sfv.clustering_agreement(res["labels"], lab, 3, 3)
        assert all(res[key][n] == ref[n] for n in ("ari", "nmi", "v_measure", "fowlkes_mallows"))
    th = chain.probs.cpu().numpy()
    assert res["prototypes"].dtype == torch.bool and np.array_equal(res["prototypes"].cpu().numpy(), th > 0.5)
    assert res["bit_reliability"].dtype == F64 and np.array_equal(res["bit_reliability"].cpu().numpy(), np.maximum(th, 1 - th))
    path = chain.path.cpu().numpy()
    cps = [t for t in range(1, F_) if path[t] != path[t - 1]]
    assert res["change_points"] == cps and res["boundaries"] == sfv.boundary_agreement(cps, [10, 30], 2)
    assert np.array_equal(res["dwell"], 1.0 / (1.0 - np.diag(chain.transmat.cpu().numpy())))
    table, K, best = res["selection"]
    assert [row["K"] for row in table] == [2, 3] and K in (2, 3)
    again = sfv.latent_code_models(model, x, range(F_), flags, u=u, n_states=4)
    assert again["bhmm"].probs.shape == (4, LD) and again["bhmm_agreement"]["contingency"].shape == (3, 4) and "selection" not in again
