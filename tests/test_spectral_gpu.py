"""GPU: the spectral kernels (csrc/spectral.hip) element by element against extended-precision values and the bounds
tests/_spectral_ref.py derives, a whole Lanczos step against the restatement, and spectral.py's solver, layout, embedding
and clustering against tests/golden/spectral.npz (tools/make_spectral_golden.py: a dense numpy.linalg.eigh, scikit-learn's
spectral_embedding and KMeans, closed forms), every output inside sentinel guard bands, every result run twice and
compared bit for bit.

Whole UMAP run (umap_project(X, 24, 0.25, init="spectral") on latent_scores.npz's 320 rows, 500 epochs).  The gate is the
one tests/test_umap_gpu.py uses, against five recorded runs of _umap_ref.layout_sequential from the spectral initial map
(seeds 42..46: cross entropy 11526.5, 11837.8, 11783.2, 11707.6, 11859.1, mean 11742.8; trustworthiness 0.82646, 0.82901,
0.81895, 0.83049, 0.82907, mean 0.82680; the initial map: 14100.4 and 0.74145): cross entropy <= 1.05 x the mean = 12330.0
and below the midpoint 12921.6, trustworthiness >= the mean - 0.005 = 0.82180.
Measured on one MI355X: cross entropy 11441.6, trustworthiness 0.82910, the map spans 5.55 x 6.23; the layout itself
(normalized_graph and the solve) took 4.3 ms of wall time."""
import os

import numpy as np
import pytest
import torch

import _spectral_ref as S
import _umap_ref as R
import sfv_amd as sfv

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-10
EIGEN_TOL = 1e-12
GUARD = 4096
SENT = {torch.float64: (torch.int64, 0x7FF8DEADDEADBEEF), torch.int32: (torch.int32, -0x21524111)}
LD = np.longdouble
call, query = sfv._lib.call, sfv._lib.query


class Guarded:
    """n elements of dtype inside GUARD sentinel elements on each side (NaN sentinels for f64), as test_umap_gpu.Guarded;
    check(written=mask) also holds the elements outside the mask to their sentinels"""

    def __init__(self, dtype, *shape):
        self.n, self.shape = int(np.prod(shape)), shape
        raw, self.sent = SENT[dtype]
        self.buf = torch.full((GUARD + self.n + GUARD,), self.sent, dtype=raw, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.n].view(dtype).view(*shape)

    def check(self, what, untouched=False, written=None):
        bits = self.buf.cpu().numpy()
        inner = np.zeros(bits.shape, dtype=bool)
        inner[GUARD:GUARD + self.n] = True
        stray = np.nonzero((bits != self.sent) & ~inner)[0]
        assert stray.size == 0, f"{what}: {stray.size} elements outside the output were written; first at {stray[0] - GUARD}"
        is_sent = (bits == self.sent)[GUARD:GUARD + self.n]
        want = np.zeros(self.n, dtype=bool) if untouched else (
            np.ones(self.n, dtype=bool) if written is None else np.broadcast_to(written, self.shape).reshape(-1))
        assert not np.any(is_sent & want), f"{what}: {int(np.sum(is_sent & want))} elements never written"
        assert not np.any(~is_sent & ~want), f"{what}: {int(np.sum(~is_sent & ~want))} elements written that must not be"
        return self.t.cpu().numpy()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _within(got, exact, bnd, what):
    err = np.abs(np.asarray(got).astype(LD) - exact)
    bad = ~(err <= bnd)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements outside the bound; worst |err|/bound = "
                           f"{float(np.max(err / bnd)):.3g}")
    return float(np.max(err / bnd)) if err.size else 0.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "spectral.npz")))


def _csr(gold, nn):
    return gold[f"indptr_{nn}"], gold[f"indices_{nn}"], gold[f"data_{nn}"]


def _ws(N, m_max, q):
    nbytes = query("rbvae_spectral_ws_bytes", N, m_max, q)
    assert nbytes > 0
    return torch.empty(nbytes // 8, dtype=torch.float64, device="cuda"), nbytes


# ---- degrees and the product ---------------------------------------------------------------------------------------------

def _rows_graph():
    """rows of 0, 1, 63, 64 and 65 entries, then rows of 2; not symmetric: the kernels do not need it"""
    r = np.random.RandomState(3)
    N, cnt = 130, [0, 1, 63, 64, 65] + [2] * 125
    cols = [np.sort(r.choice(N, c, replace=False)) for c in cnt]
    indptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    indices = np.concatenate(cols).astype(np.int32)
    return indptr, indices, (0.1 + r.rand(len(indices))).astype(np.float32)


def _stray_columns():
    ip, ix, w = _rows_graph()
    ix = ix.copy()
    ix[[3, 70, 140]] = [130, -1, 1 << 30]
    return ip, ix, w


def _degree_and_product(csr, what):
    ip, ix, w = csr
    N = len(ip) - 1
    d_csr = (_dev(ip), _dev(ix), _dev(w))
    out = []
    for _ in range(2):
        deg, isd, y = Guarded(torch.float64, N), Guarded(torch.float64, N), Guarded(torch.float64, N)
        call("rbvae_spectral_degree", *d_csr, N, deg.t, isd.t)
        x = np.random.RandomState(N % 1000).randn(N)
        call("rbvae_spectral_matvec", *d_csr, isd.t, N, _dev(x), y.t)
        out.append((deg.check("deg"), isd.check("isd"), y.check("y")))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(*out)), f"{what}: two runs differ"
    deg, isd, y = out[0]
    rdeg, risd, b_deg, b_isd = S.degree(*csr)
    ok = (ix.astype(np.int64) >= 0) & (ix.astype(np.int64) < N)
    exact = np.zeros(N, dtype=LD)
    np.add.at(exact, S.rows_of(ip), np.where(ok, w.astype(LD), LD(0)))
    zero = exact == 0
    assert np.all(deg[zero] == 0) and np.all(isd[zero] == 0) and np.all(y[zero] == 0)
    wd = _within(deg, exact, b_deg + S.TINY, f"deg ({what})")
    wi = _within(isd, np.where(zero, LD(0), 1 / np.sqrt(np.where(zero, LD(1), exact))), b_isd + S.TINY, f"isd ({what})")
    ry, b_y = S.matvec(*csr, isd, x)
    wy = _within(y, S.matvec_exact(*csr, isd, x), b_y, f"y ({what})")
    assert np.isfinite(y).all()
    print(f"{what}: N {N}, largest row {np.diff(ip).max()}, worst |err|/bound deg {wd:.3g}, isd {wi:.3g}, y {wy:.3g}; "
          f"bit-equal to the restatement: deg {np.array_equal(deg, rdeg)}, isd {np.array_equal(isd, risd)}, "
          f"y {np.array_equal(y, ry)}")


@pytest.mark.parametrize("what", ["rows", "stray columns", "star", "two vertices", "fixture", "path at the cap"])
def test_degree_and_product(gold, what):
    csr = {"rows": _rows_graph, "stray columns": _stray_columns, "star": lambda: R.star_graph(200),
           "two vertices": lambda: S.to_csr([[0.0, 0.5], [0.5, 0.0]]), "fixture": lambda: _csr(gold, 24),
           "path at the cap": lambda: S.path_graph(1 << 20)}[what]()
    if what == "star":
        assert np.diff(csr[0]).max() == 199                 # four chunks of 64, the last one partial
    _degree_and_product(csr, what)


# ---- dot products and the update -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1023, 1024, 1025, 3073])
@pytest.mark.parametrize("nv", [1, 2, 64, 65])
def test_dots_and_update(N, nv):
    assert query("rbvae_spectral_block_rows") == S.BLOCK
    r = np.random.RandomState(N + nv)
    V, w, cc = r.randn(nv, N), r.randn(N), r.randn(nv)
    ws, nbytes = _ws(N, max(nv - 1, 1), 0)
    out = []
    for _ in range(2):
        c, wg = Guarded(torch.float64, nv), Guarded(torch.float64, N)
        wg.t.copy_(_dev(w))
        call("rbvae_spectral_dots", _dev(V), nv, N, _dev(w), c.t, ws, nbytes)
        call("rbvae_spectral_update", _dev(V), nv, N, _dev(cc), wg.t)
        out.append((c.check("c"), wg.check("w")))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(*out)), "two runs differ"
    rc, b_c = S.dots(V, w)
    rw, b_w = S.update(V, cc, w)
    wc = _within(out[0][0], (V.astype(LD) * w.astype(LD)).sum(1), b_c, "c")
    ww = _within(out[0][1], w.astype(LD) - (cc.astype(LD)[:, None] * V.astype(LD)).sum(0), b_w, "w")
    print(f"N {N}, nv {nv}: worst |err|/bound c {wc:.3g}, w {ww:.3g}; bit-equal to the restatement: "
          f"{np.array_equal(out[0][0], rc)}, {np.array_equal(out[0][1], rw)}")


# ---- one step ------------------------------------------------------------------------------------------------------------

M_STEP = 72


@pytest.fixture(scope="module")
def basis(gold):
    """72 restated steps on the fixture graph with the trivial vector locked (q = 1)"""
    csr = _csr(gold, 24)
    return S.lanczos(*csr, 3, tol=0.0, max_steps=M_STEP, locked=S.trivial_vector(*csr), keep_basis=True)


@pytest.mark.parametrize("j,noise", [(0, 0.0), (70, 0.0), (5, 1e-6)])
def test_one_step(gold, basis, j, noise):
    """j = 70: more vectors than a wave has lanes.  noise: a basis orthonormal only to 1e-6, where the second pass's
    coefficient on v_j is about 1e-6 and an alpha taken from the first pass alone is far outside the bound"""
    csr, q, N = _csr(gold, 24), 1, 320
    V = basis["V"][:q + j + 1].copy()
    if noise:
        V += noise * np.random.RandomState(5).randn(*V.shape)
    isd = basis["isd"]
    ref = S.step(csr, isd, np.concatenate([V, np.zeros((1, N))]), q, j)
    d_csr = (_dev(csr[0]), _dev(csr[1]), _dev(csr[2]))
    ws, nbytes = _ws(N, M_STEP, q)
    out = []
    for _ in range(2):
        Vg = Guarded(torch.float64, q + M_STEP + 1, N)
        al, be, st = Guarded(torch.float64, M_STEP), Guarded(torch.float64, M_STEP), Guarded(torch.int32, 2)
        Vg.t[:q + j + 1].copy_(_dev(V))
        st.t.zero_()
        call("rbvae_spectral_step", *d_csr, _dev(isd), N, Vg.t, q, j, M_STEP, al.t, be.t, st.t, ws, nbytes)
        rows = (np.arange(q + M_STEP + 1) <= q + j + 1)[:, None]
        only_j = np.arange(M_STEP) == j
        out.append((Vg.check("V", written=rows), al.check("alpha", written=only_j), be.check("beta", written=only_j),
                    st.check("state")))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(*out)), "two runs differ"
    Vd, al, be, st = out[0]
    assert np.array_equal(_bits(Vd[:q + j + 1]), _bits(V)), "the basis was written"
    assert st.tolist() == [0, j + 1]
    assert abs(al[j] - ref["alpha"]) <= ref["D_a"] and abs(be[j] - ref["beta"]) <= ref["D_b"]
    assert np.all(np.abs(Vd[q + j + 1] - ref["v"]) <= ref["D_v"])
    print(f"step j = {j}: alpha {al[j]:.6f} (|err| {abs(al[j] - ref['alpha']):.3g}, bound {ref['D_a']:.3g}), beta "
          f"{be[j]:.6f} (|err| {abs(be[j] - ref['beta']):.3g}, bound {ref['D_b']:.3g}), v |err| "
          f"{np.abs(Vd[q + j + 1] - ref['v']).max():.3g}, bound {ref['D_v']:.3g}")
    if noise:
        bad = S.step(csr, isd, np.concatenate([V, np.zeros((1, N))]), q, j, defect="alpha_first_pass_only")
        assert abs(bad["alpha"] - al[j]) > ref["D_a"]


def test_steps_after_breakdown_write_nothing():
    """K_8 from a start vector: beta_1 is rounding, the third and fourth enqueued steps return at once"""
    csr = S.complete_graph(8)
    N, m_max = 8, 6
    d_csr = (_dev(csr[0]), _dev(csr[1]), _dev(csr[2]))
    isd = _dev(S.degree(*csr)[1])
    Vg = Guarded(torch.float64, m_max + 1, N)
    al, be, st = Guarded(torch.float64, m_max), Guarded(torch.float64, m_max), Guarded(torch.int32, 2)
    Vg.t[0].copy_(_dev(S.unit(np.random.RandomState(0).uniform(-1, 1, N))))
    st.t.zero_()
    ws, nbytes = _ws(N, m_max, 0)
    for j in range(4):
        call("rbvae_spectral_step", *d_csr, isd, N, Vg.t, 0, j, m_max, al.t, be.t, st.t, ws, nbytes)
    assert st.check("state").tolist() == [1, 2]
    Vg.check("V", written=(np.arange(m_max + 1) <= 2)[:, None])
    b = be.check("beta", written=np.arange(m_max) < 2)
    al.check("alpha", written=np.arange(m_max) < 2)
    assert b[0] > 0.1 and b[1] <= S.BREAKDOWN


# ---- whole solves --------------------------------------------------------------------------------------------------------

def _graph(csr):
    return sfv.normalized_graph(*csr)


def _host_residuals(csr, isd, r):
    vec = r.vectors.cpu().numpy()
    return np.array([np.linalg.norm(S.matvec(*csr, isd, vec[:, i])[0] - (1 - r.eigenvalues[i]) * vec[:, i])
                     for i in range(vec.shape[1])])


def _same(a, b):
    return (np.array_equal(_bits(a.eigenvalues), _bits(b.eigenvalues)) and torch.equal(a.vectors, b.vectors)
            and np.array_equal(_bits(a.residuals), _bits(b.residuals)) and (a.steps, a.why) == (b.steps, b.why))


@pytest.mark.parametrize("nn", [24, 15])
def test_solve_against_dense_eigh(gold, nn):
    csr = _csr(gold, nn)
    N, max_deg = 320, int(np.diff(csr[0]).max())
    g = _graph(csr)
    assert g.n_components == 1
    rdeg, risd, b_deg, b_isd = S.degree(*csr)
    assert np.all(np.abs(g.deg.cpu().numpy() - rdeg) <= 2 * b_deg)     # each side within b of the exact value
    assert np.all(np.abs(g.isd.cpu().numpy() - risd) <= 2 * b_isd)
    q0 = sfv.spectral.trivial_vector(g)
    r = sfv.lanczos_eigsh(g, 8, locked=q0)
    assert _same(r, sfv.lanczos_eigsh(g, 8, locked=q0)), "two runs differ"
    assert r.converged and r.why == "tol" and r.steps % 8 == 0 and r.vectors.shape == (N, 8)
    vec = r.vectors.cpu().numpy()
    ge = S.eigenvalue_gate(r.eigenvalues, gold[f"lam_{nn}"][1:9], TOL, N)
    gv = S.vector_gate(vec, r.residuals, gold[f"vec_{nn}"], gold[f"lam_{nn}"], range(1, 9), N)
    go = S.orth_gate(vec, 1, r.steps)
    host = _host_residuals(csr, g.isd.cpu().numpy(), r)
    B = -(-N // S.BLOCK)
    round_bound = 2 * (9 + -(-max_deg // 64)) * S.U * np.sqrt(N) + (16 + B) * S.U * r.residuals
    print(f"n_neighbors {nn}: {r.steps} steps, worst |err|/bound eigenvalues {ge:.3g}, vectors {gv:.3g}, orthonormality "
          f"{go:.3g}; residuals device {r.residuals.max():.3g}, host {host.max():.3g}")
    assert ge <= 1 and gv <= 1 and go <= 1
    assert np.all(host <= r.residuals + round_bound) and np.all(host <= S.residual_cap(TOL, 1, r.steps, N, max_deg))
    big = np.argmax(np.abs(vec), axis=0)
    assert np.all(vec[big, np.arange(8)] > 0)
    lr = sfv.spectral._layout(g, 2)
    assert torch.equal(lr.vectors, sfv.spectral_layout(g, 2)) and lr.steps < r.steps
    assert S.vector_gate(lr.vectors.cpu().numpy(), lr.residuals, gold[f"vec_{nn}"], gold[f"lam_{nn}"], (1, 2), N) <= 1
    emb = sfv.spectral_embedding(g, 8)
    ref = gold[f"sk_emb_{nn}"]
    bound = float(g.isd.max()) * S.davis_kahan(r.residuals + EIGEN_TOL, S.gaps(gold[f"lam_{nn}"], range(1, 9)), N)
    gs = float(np.max(np.linalg.norm(emb.cpu().numpy() - ref, axis=0) / bound))
    print(f"n_neighbors {nn}: worst |err|/bound against sklearn.manifold.spectral_embedding {gs:.3g}")
    assert emb.shape == ref.shape and gs <= 1
    assert torch.equal(emb, sfv.spectral_embedding(g, 8))


@pytest.mark.parametrize("n", [64, 1000])
def test_path_graph_closed_form(n):
    csr = S.path_graph(n)
    g = _graph(csr)
    r = sfv.lanczos_eigsh(g, 4)
    assert S.eigenvalue_gate(r.eigenvalues, S.path_eigenvalues(n, 4), TOL, n) <= 1
    assert np.all(_host_residuals(csr, g.isd.cpu().numpy(), r) <= S.residual_cap(TOL, 0, r.steps, n, 2))
    assert S.orth_gate(r.vectors.cpu().numpy(), 0, r.steps) <= 1
    print(f"path {n}: {r.steps} steps, {r.why}, residuals {r.residuals.max():.3g}")
    if n == 64:
        r = sfv.lanczos_eigsh(g, n - 1, locked=sfv.spectral.trivial_vector(g), max_steps=n - 1)
        assert r.why == "invariant" and r.converged and r.steps == n - 1 and r.vectors.shape == (n, n - 1)
        assert S.eigenvalue_gate(r.eigenvalues, S.path_eigenvalues(n, n)[1:], TOL, n) <= 1
        assert S.orth_gate(r.vectors.cpu().numpy(), 1, r.steps) <= 1


def test_complete_graph_breaks_down():
    g = _graph(S.complete_graph(8))
    r = sfv.lanczos_eigsh(g, 2)
    assert r.converged and r.why == "invariant" and r.steps == 2
    assert S.eigenvalue_gate(r.eigenvalues, [0.0, 8.0 / 7.0], TOL, 8) <= 1
    r3 = sfv.lanczos_eigsh(g, 3)
    assert not r3.converged and r3.why == "invariant" and r3.vectors.shape == (8, 2) and len(r3.eigenvalues) == 2
    assert np.array_equal(_bits(r3.eigenvalues), _bits(r.eigenvalues)) and torch.equal(r3.vectors, r.vectors)


def test_cycle_is_regular():
    """q0 is locked, so the all-ones eigenvector cannot end the run at step 1; 1 - cos(2 pi / 6) is double: only the
    eigenvalue and the residual are held"""
    csr = S.cycle_graph(6)
    g = _graph(csr)
    r = sfv.spectral._layout(g, 2)
    assert r.steps >= 2 and r.vectors.shape[0] == 6
    assert abs(r.eigenvalues[0] - (1 - np.cos(2 * np.pi / 6))) <= TOL + 6 * 2.0 ** -52
    assert _host_residuals(csr, g.isd.cpu().numpy(), r)[0] <= S.residual_cap(TOL, 1, r.steps, 6, 2)


def test_disconnected_graph():
    g = _graph(S.two_cliques(5))
    assert g.n_components == 2
    with pytest.raises(ValueError, match="2 connected components"):
        sfv.spectral_layout(g, 2)
    r = np.random.RandomState(0)
    X = np.concatenate([r.randn(20, 3), 100.0 + r.randn(20, 3)]).astype(np.float32)
    a = sfv.umap_project(_dev(X), 5, n_epochs=20, init="spectral")
    b = sfv.umap_project(_dev(X), 5, n_epochs=20, init="pca")
    assert a.init == "pca" and b.init == "pca" and torch.equal(a.embedding, b.embedding)
    with pytest.raises(ValueError, match="init"):
        sfv.umap_project(_dev(X), 5, n_epochs=20, init="random")


def test_refused_arguments_write_nothing(gold):
    csr = _csr(gold, 24)
    N = 320
    d_csr = (_dev(csr[0]), _dev(csr[1]), _dev(csr[2]))
    isd = _dev(S.degree(*csr)[1])
    V = Guarded(torch.float64, 12, N)
    al, be, st = Guarded(torch.float64, 4), Guarded(torch.float64, 4), Guarded(torch.int32, 2)
    Y, res, deg = Guarded(torch.float64, 33, N), Guarded(torch.float64, 33), Guarded(torch.float64, N)
    ws, nbytes = _ws(N, 1024, 8)
    s = torch.zeros((4, 33), dtype=torch.float64, device="cuda")

    def step(q=0, j=0, m_max=2, nb=nbytes, n=N):
        call("rbvae_spectral_step", *d_csr, isd, n, V.t, q, j, m_max, al.t, be.t, st.t, ws, nb)

    assert query("rbvae_spectral_ok", N, 1025, 0) == 0 and query("rbvae_spectral_ok", N, 4, 9) == 0
    assert query("rbvae_spectral_ok", 1, 4, 0) == 0 and query("rbvae_spectral_ok", (1 << 20) + 1, 4, 0) == 0
    assert query("rbvae_spectral_ws_bytes", N, 1025, 0) == 0
    for match, kw in (("m_max=1025", dict(m_max=1025)), ("q=9", dict(q=9)), ("N=1,", dict(n=1))):
        with pytest.raises(RuntimeError, match=match):
            step(**kw)
    with pytest.raises(ValueError, match="workspace"):
        step(nb=query("rbvae_spectral_ws_bytes", N, 2, 0) - 8)
    with pytest.raises(ValueError, match="j=2"):
        step(j=2)
    with pytest.raises(RuntimeError, match="cols=33"):
        call("rbvae_spectral_ritz", V.t, 0, 4, N, s, 33, Y.t)
    with pytest.raises(RuntimeError, match="cols=33"):
        call("rbvae_spectral_residuals", *d_csr, isd, N, Y.t, 33, res.t, res.t, ws, nbytes)
    with pytest.raises(RuntimeError, match="N=1,"):
        call("rbvae_spectral_degree", *d_csr, 1, deg.t, deg.t)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_spectral_matvec", *d_csr, isd, N, None, deg.t)
    for gd, name in ((V, "V"), (al, "alpha"), (be, "beta"), (st, "state"), (Y, "Y"), (res, "res"), (deg, "deg")):
        gd.check(name, untouched=True)
    g = _graph(csr)
    for kw in (dict(k=0), dict(k=3, max_steps=2), dict(k=2, max_steps=1025), dict(k=2, locked=np.zeros((9, N)))):
        with pytest.raises(ValueError):
            sfv.lanczos_eigsh(g, **kw)
    with pytest.raises(ValueError, match="ascend"):
        sfv.normalized_graph(np.array([0, 2, 2]), np.array([1, 0]), np.array([1.0, 1.0], dtype=np.float32))
    with pytest.raises(ValueError, match="square"):
        sfv.normalized_graph(np.array([0, 1, 2]), np.array([1, 2]), np.array([1.0, 1.0], dtype=np.float32))


# ---- clustering ----------------------------------------------------------------------------------------------------------

def test_spectral_clustering_against_the_reference_pipeline(gold):
    g = _graph(_csr(gold, 24))
    assert len(gold["cl_K"]) >= 2
    embeddings = {}
    for K, seed, want in zip(gold["cl_K"].tolist(), gold["cl_seed"].tolist(), gold["cl_labels"]):
        km, emb = sfv.spectral_clustering(g, K, seed=seed)
        if K in embeddings:
            assert torch.equal(emb, embeddings[K]), "two runs differ"
        embeddings[K] = emb
        assert emb.shape == (320, K) and emb.dtype == torch.float64
        labels = km.labels.cpu().numpy()
        assert np.array_equal(labels, want), f"K = {K}, seed {seed}: {int((labels != want).sum())} rows differ"
        plain = sfv.kmeans(emb.float().contiguous(), K, seed=seed)
        assert torch.equal(plain.labels, km.labels) and plain.n_iter == km.n_iter


def test_latent_spectral():
    F_, RES, LDIM = 48, 64, 16
    torch.manual_seed(0)
    model = sfv.Seq2SeqBinaryVAE(3, 3, LDIM, LDIM, variant="contrastive", input_hw=(RES, RES),
                                 compute_dtype="f32").cuda().eval()
    x = torch.rand(F_, 3, RES, RES, generator=torch.Generator().manual_seed(1)).cuda()
    u = torch.rand(F_, LDIM, generator=torch.Generator().manual_seed(2))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # a random model's graph may have several components
        out = sfv.latent_spectral(model, x, range(F_), [10, 30], n_neighbors=10, u=u)
        again = sfv.latent_spectral(model, x, range(F_), [10, 30], n_neighbors=10, u=u)
    assert sorted(out) == ["agreement", "cluster_embedding", "clustering", "embedding", "graph", "labels", "latents"]
    assert tuple(out["embedding"].shape) == (F_, 2) and tuple(out["cluster_embedding"].shape) == (F_, 3)
    assert torch.equal(out["embedding"], again["embedding"]) and torch.equal(out["clustering"].labels,
                                                                             again["clustering"].labels)
    assert -1.0 <= out["agreement"]["ari"] <= 1.0 and out["agreement"]["contingency"].shape == (3, 3)
    assert out["labels"].tolist() == [sfv.assign_label(f, [10, 30]) for f in range(F_)]


# ---- UMAP from the spectral layout ---------------------------------------------------------------------------------------

def test_umap_project_spectral_init(gold):
    """Measured on one MI355X: cross entropy 11441.6 (bounds 12330.0 and 12921.6), trustworthiness 0.82910 (bound
    0.82180); see the module's docstring"""
    from sklearn.manifold import trustworthiness
    X = np.load(os.path.join(GOLDEN, "latent_scores.npz"))["X"]
    Xd = _dev(X)
    t = {}
    r1 = sfv.umap_project(Xd, 24, 0.25, init="spectral", timings=t)
    r2 = sfv.umap_project(Xd, 24, 0.25, init="spectral")
    assert r1.init == "spectral" and "spectral" in t and torch.equal(r1.embedding, r2.embedding), "two runs differ"
    graph = sfv.fuzzy_graph(*sfv.knn_graph(Xd, 23), 24)
    lay = sfv.spectral_layout(graph, 2)
    Y0 = sfv.projection.umap_initial_map(lay.cpu().numpy(), 42)
    res = sfv.umap_optimise(_dev(Y0), graph, a=r1.a, b=r1.b)
    assert torch.equal(res.embedding, r1.embedding) and res.init == "given"
    assert np.abs(Y0.astype(np.float64) - gold["Y0"]).max() <= 1e-4     # the recorded start, up to the noise's own scale
    Ya = r1.embedding.cpu().numpy()
    a, b = float(gold["a"]), float(gold["b"])
    assert abs(r1.a - a) < 1e-9 and abs(r1.b - b) < 1e-9
    ce = R.cross_entropy(Ya, *_csr(gold, 24), a, b)
    trust = trustworthiness(X, Ya, n_neighbors=24)
    seq_ce, seq_trust, ce0 = float(gold["seq_ce"].mean()), float(gold["seq_trust"].mean()), float(gold["ce_init"])
    print(f"spectral start: cross entropy {ce:.1f} (sequential mean {seq_ce:.1f}, initial map {ce0:.1f}), trustworthiness "
          f"{trust:.5f} (sequential mean {seq_trust:.5f}), span {np.ptp(Ya, axis=0)}, spectral {t['spectral']:.1f} ms")
    assert ce <= 1.05 * seq_ce
    assert ce < 0.5 * (seq_ce + ce0)
    assert trust >= seq_trust - 0.005


def test_umap_project_pca_spelled_out():
    Xp = _dev(np.load(os.path.join(GOLDEN, "projection.npz"))["X"])
    Y0 = _dev(np.load(os.path.join(GOLDEN, "umap.npz"))["Y0"])
    a, b, c = (sfv.umap_project(Xp, 24, 0.25, init=i) for i in (None, "pca", Y0))
    assert (a.init, b.init, c.init) == ("pca", "pca", "given")
    assert torch.equal(a.embedding, b.embedding) and torch.equal(a.embedding, c.embedding)
