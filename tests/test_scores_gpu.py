"""GPU: the score kernels (csrc/scores.hip) against tests/_scores_ref.py's f64 restatement inside sentinel guard bands
-- ranks equal wherever they are decided, Euclidean sums element-wise within the bound its docstring derives, Hamming sums
integer-exact -- and scores.py end to end against the scikit-learn fixture tests/golden/latent_scores.npz
(tools/make_scores_golden.py).

Measured on one MI355X: no undecided rank entry on any case and every rank equal; trustworthiness and continuity on the
fixture differ from scikit-learn's by 0.0 at k = 5, 24 and 91; the Euclidean sums' worst |err| / bound is 0.173 at
(65, 3, 4) and 0.06 to 0.08 on the cases of 50 and 128 values; silhouette samples within 8.4e-16 of scikit-learn's."""
import os

import numpy as np
import pytest
import torch

import _scores_ref as R
import sfv_amd as sfv

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "latent_scores.npz")
GUARD = 4096
SENT = {torch.float64: (torch.int64, 0x7FF8DEADDEADBEEF), torch.int32: (torch.int32, -0x21524111)}
LS_CHUNK = 4096                         # f64 values of j rows per LDS chunk of the Euclidean sums


class Guarded:
    """n elements of dtype inside GUARD sentinel elements on each side (a NaN sentinel for f64)"""

    def __init__(self, dtype, *shape):
        self.n = int(np.prod(shape))
        raw, self.sent = SENT[dtype]
        self.buf = torch.full((GUARD + self.n + GUARD,), self.sent, dtype=raw, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.n].view(dtype).view(*shape)

    def check(self, what, untouched=False):
        bits = self.buf.cpu().numpy()
        inner = np.zeros(bits.shape, dtype=bool)
        inner[GUARD:GUARD + self.n] = True
        stray = np.nonzero((bits != self.sent) & ~inner)[0]
        assert stray.size == 0, f"{what}: {stray.size} elements outside the output were written; first at {stray[0] - GUARD}"
        unwritten = np.nonzero((bits == self.sent) & inner)[0]
        if untouched:
            assert unwritten.size == self.n, f"{what}: a refused call wrote {self.n - unwritten.size} elements"
        else:
            assert unwritten.size == 0, f"{what}: {unwritten.size} elements never written; first at {unwritten[0] - GUARD}"
        return self.t.cpu().numpy()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLD))
    g["DX"] = R.sqdist(g["X"])
    return g


def _sqdist_device(X, rows):
    """_projection_ref.sqdist for a block of rows, in torch's element-wise f64 operations on the device: the same
    arithmetic in the same order (l ascending, each square rounded once)"""
    D = torch.zeros((len(rows), X.shape[0]), dtype=torch.float64, device="cuda")
    for l in range(X.shape[1]):
        df = X[rows, l][:, None] - X[None, :, l]
        D += df * df
    return D


# ---- ranks -----------------------------------------------------------------------------------------------------------------

def _ranks_guarded(X, nbr):
    N, Ld = X.shape
    k = nbr.shape[1]
    rank, excess = Guarded(torch.int32, N, k), Guarded(torch.int32, N)
    sfv._lib.call("rbvae_nbr_ranks", _dev(X), N, Ld, _dev(nbr), k, rank.t, excess.t)
    return rank.check("rank"), excess.check("excess")


def _ranks_ref_blocked(X, nbr, block=512):
    """R.ranks for sizes whose N x N matrix does not belong on the host, a block of rows at a time on the device"""
    Xd, nb = torch.from_numpy(X).cuda().double(), torch.from_numpy(nbr).cuda().long()
    N, k = nb.shape
    m = torch.arange(N, device="cuda")[None, :]
    out_r, out_ok = [], []
    for i0 in range(0, N, block):
        rows = torch.arange(i0, min(N, i0 + block), device="cuda")
        D = _sqdist_device(Xd, rows)
        other = m != rows[:, None]
        rk = torch.empty((len(rows), k), dtype=torch.int32, device="cuda")
        ok = torch.empty((len(rows), k), dtype=torch.bool, device="cuda")
        for r in range(k):
            j = nb[rows, r][:, None]
            dj = torch.gather(D, 1, j)
            before = ((D < dj) | ((D == dj) & (m < j))) & other
            rk[:, r] = 1 + before.sum(1)
            ok[:, r] = ~(((D - dj).abs() < 1e-12 * dj) & (D != dj) & other).any(1)
        out_r.append(rk)
        out_ok.append(ok)
    return torch.cat(out_r).cpu().numpy(), torch.cat(out_ok).cpu().numpy()


RANK_CASES = [(2, 1, 1), (65, 3, 31), (257, 50, 24), (320, 50, 5), (320, 50, 24), (700, 128, 5), (4100, 2, 24), (16384, 2, 3)]


@pytest.mark.parametrize("N,Ld,k", RANK_CASES)
def test_ranks(gold, N, Ld, k):
    fixture = N == 320
    if fixture:
        X, nbr = gold["X"], R.knn(gold["Y"], k)[0]          # the neighbours in the map, as trustworthiness takes them
    else:
        X, nbr = R.soft_rows(N, Ld, N + Ld), R.random_neighbours(N, k, N + k)
    assert sfv._lib.query("rbvae_nbr_ranks_ok", N, Ld, k) == 1
    rank, excess = _ranks_guarded(X, nbr)
    if N > 1000:
        ref, decided = _ranks_ref_blocked(X, nbr)
    else:
        ref, _, decided = R.ranks(X, nbr, D=gold["DX"] if fixture else None)
    assert decided.mean() >= 0.99 and (decided.all() or not fixture)
    assert np.array_equal(rank[decided], ref[decided])
    assert rank.min() >= 1 and rank.max() <= N - 1
    assert np.array_equal(excess, np.maximum(rank.astype(np.int64) - k, 0).sum(1))
    print(f"ranks ({N}, {Ld}, {k}): {int((~decided).sum())} undecided entries, ranks {rank.min()}..{rank.max()}, "
          f"sum of excess {int(excess.astype(np.int64).sum())}")
    rank2, excess2 = _ranks_guarded(X, nbr)
    assert np.array_equal(rank, rank2) and np.array_equal(excess, excess2), "two runs differ"


def test_ranks_of_duplicated_rows():
    """hard codes as floats: integer distances, zeros and exact ties, ordered by the index on both sides"""
    X = R.hard_codes()
    D = R.sqdist(X)
    for nbr in (R.knn(X, 64, D=D)[0], R.random_neighbours(len(X), 9, 2)):
        ref, ref_ex, decided = R.ranks(X, nbr, D=D)
        rank, excess = _ranks_guarded(X, nbr)
        assert decided.all() and np.array_equal(rank, ref) and np.array_equal(excess, ref_ex)
    assert np.array_equal(rank, R.ranks(X, nbr, D=D)[0]) and not np.array_equal(rank, R.ranks(X, nbr, "tie_high", D=D)[0])


def test_ranks_of_own_neighbours(gold):
    """with the neighbours of X itself rank[i][r] = r + 1 everywhere: the two kernels order a row identically"""
    X = _dev(gold["X"])
    for k in (5, 24, 91):
        idx, _ = sfv.knn_graph(X, k)
        rank, excess = sfv.neighbour_ranks(X, idx)
        assert torch.equal(rank, torch.arange(1, k + 1, dtype=torch.int32, device="cuda").expand(320, k))
        assert int(excess.abs().max()) == 0
        assert sfv.trustworthiness(X, X, k) == 1.0
    Xc = _dev(R.hard_codes())                               # and where most distances are tied
    idx, _ = sfv.knn_graph(Xc, 64)
    assert torch.equal(sfv.neighbour_ranks(Xc, idx)[0], torch.arange(1, 65, dtype=torch.int32, device="cuda").expand(160, 64))


def test_ranks_skip_entries_that_are_no_row():
    N, Ld, k = 257, 50, 24
    X, nbr = R.soft_rows(N, Ld, N + Ld), R.random_neighbours(N, k, N + k)
    rank, _ = _ranks_guarded(X, nbr)
    bad = nbr.copy()
    bad[3, 0], bad[3, 5], bad[100, 23], bad[256, 7] = 0x7FFFFFFF, -1, 100, N
    bad[17, :] = 0x7FFFFFFF                                 # a row rbvae_knn could not fill at all
    hit = bad != nbr
    rank_b, excess_b = _ranks_guarded(X, bad)
    assert np.all(rank_b[hit] == -1) and np.array_equal(rank_b[~hit], rank[~hit])
    assert np.array_equal(excess_b, np.where(rank_b > k, rank_b - k, 0).sum(1)) and excess_b[17] == 0


def test_ranks_refused_shapes_write_nothing():
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")       # noqa: E731
    zi = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")        # noqa: E731
    rank, excess = Guarded(torch.int32, 4, 2), Guarded(torch.int32, 4)
    for N, Ld, k, match in ((4, 129, 2, "L=129"), (4, 3, 4, "k=4"), (1, 3, 1, "N=1"), (4, 3, 0, "k=0"), (16385, 2, 2, "N=16385")):
        assert sfv._lib.query("rbvae_nbr_ranks_ok", N, Ld, k) == 0
        with pytest.raises(ValueError, match=match):
            sfv._lib.call("rbvae_nbr_ranks", z(4, 129), N, Ld, zi(4, 4), k, rank.t, excess.t)
    with pytest.raises(ValueError, match="null"):
        sfv._lib.call("rbvae_nbr_ranks", z(4, 3), 4, 3, None, 2, rank.t, excess.t)
    with pytest.raises(ValueError, match="k=129"):
        sfv._lib.call("rbvae_nbr_ranks", z(200, 3), 200, 3, zi(200, 129), 129, rank.t, excess.t)
    rank.check("rank", untouched=True)
    excess.check("excess", untouched=True)


@pytest.mark.parametrize("k", [5, 24, 91])
def test_trustworthiness_against_sklearn(gold, k):
    X, Y = _dev(gold["X"]), _dev(gold["Y"])
    t, c = sfv.trustworthiness(X, Y, k), sfv.continuity(X, Y, n_neighbors=k)
    print(f"k = {k}: trustworthiness {t:.6f} (scikit-learn {float(gold[f'trust_{k}']):.6f}), continuity {c:.6f} "
          f"({float(gold[f'cont_{k}']):.6f})")
    assert abs(t - float(gold[f"trust_{k}"])) <= 1e-15
    assert abs(c - float(gold[f"cont_{k}"])) <= 1e-15


# ---- Euclidean sums ----------------------------------------------------------------------------------------------------------

def _sums_guarded(entry, dtype, X, lab, S):
    N, Ld = X.shape
    order, seg = R.group(lab, S)
    sums = Guarded(dtype, N, S)
    sfv._lib.call(entry, _dev(X), N, Ld, _dev(order), _dev(seg), S, sums.t)
    return sums.check(f"sums ({N}, {Ld}, {S})")


SUM_CASES = [(2, 1, 2), (65, 3, 4), (257, 50, 8), (320, 50, 8), (320, 50, 11), (700, 128, 17), (4100, 50, 17)]


@pytest.mark.parametrize("N,Ld,S", SUM_CASES)
def test_dist_sums(gold, N, Ld, S):
    D = None
    if N == 320:
        X, lab, D = gold["X"], gold["lab" if S == 8 else "lab_edge"].astype(np.int64), gold["DX"]
    else:
        X = R.soft_rows(N, Ld, N + Ld)
        lab = R.edge_states(N, S, N) if N == 257 else np.random.RandomState(N).permutation(N) % S
        if N == 2:
            lab = np.array([1, 0])
    n = np.bincount(lab, minlength=S)
    if N == 257:
        assert n[1] == 0 and n[S - 1] == 1
    if N == 4100:                                           # several LDS chunks per state, the last one partial
        per = LS_CHUNK // ((Ld + 7) // 8 * 8)
        assert np.all(n > 2 * per) and np.all(n % per != 0)
        Xd = torch.from_numpy(X).cuda().double()
        D = torch.cat([_sqdist_device(Xd, torch.arange(i0, min(N, i0 + 1024), device="cuda"))
                       for i0 in range(0, N, 1024)]).cpu().numpy()
    assert sfv._lib.query("rbvae_label_sums_ok", N, Ld, S) == 1
    got = _sums_guarded("rbvae_label_dist_sums", torch.float64, X, lab, S)
    ref = R.dist_sums(X, lab, S, D=D)
    w = R.within(got, ref, R.sum_bound(Ld, lab, S, ref), f"sums ({N}, {Ld}, {S})")
    print(f"Euclidean sums ({N}, {Ld}, {S}): states of {n.min()}..{n.max()} rows, worst |err|/bound {w:.3g}")
    assert np.all(got[:, n == 0] == 0.0)
    again = _sums_guarded("rbvae_label_dist_sums", torch.float64, X, lab, S)
    assert np.array_equal(got.view(np.int64), again.view(np.int64)), "two runs differ"
    if N == 257:                                            # entries of `order` that are no row are skipped
        order, seg = R.group(lab, S)
        order[[4, 200]] = [N, -1]
        drop = np.ones(N, dtype=bool)
        drop[R.group(lab, S)[0][[4, 200]]] = False
        sums = Guarded(torch.float64, N, S)
        sfv._lib.call("rbvae_label_dist_sums", _dev(X), N, Ld, _dev(order), _dev(seg), S, sums.t)
        ref2 = R.dist_sums(X[drop], lab[drop], S)
        got2 = sums.check("sums with skipped entries")[drop]
        R.within(got2, ref2, R.sum_bound(Ld, lab[drop], S, ref2), "sums with skipped entries")


# ---- Hamming sums ------------------------------------------------------------------------------------------------------------

def _codes(N, Ld, S, seed):
    """hard codes drawn from a few distinct rows (exact duplicates); states 0 and 1 hold one and the same code, so their
    rows have a = b = 0"""
    r = np.random.RandomState(seed)
    C = r.randint(0, 2, (12, Ld))[r.randint(0, 12, N)].astype(np.float32)
    lab = r.randint(0, S, N)
    lab[:S] = np.arange(S)
    lab[7] = 2
    C[lab <= 1] = C[0]
    C[C > 0.5] = 0.501 + r.rand(int((C > 0.5).sum())).astype(np.float32) * 0.5             # the threshold is 0.5, not 1
    C[7, 0] = 0.5                                           # exactly 0.5 is a 0 bit
    return C, lab


@pytest.mark.parametrize("Ld", [1, 32, 33, 50, 64, 65, 128])
def test_hamming_sums(Ld):
    N, S = 300, 5
    C, lab = _codes(N, Ld, S, Ld)
    got = _sums_guarded("rbvae_label_hamming_sums", torch.int32, C, lab, S)
    ref = R.hamming_sums(C, lab, S)
    assert np.array_equal(got, ref)
    assert ref.max() > 0
    s = sfv.silhouette_samples(_dev(C), lab, S, metric="hamming")
    assert np.isfinite(s).all() and np.abs(s - R.silhouette(ref, lab, S)).max() <= 1e-15
    flat = lab <= 1                                         # a = b = 0 -> 0, scikit-learn's nan_to_num
    assert flat.any() and np.all(s[flat] == 0.0) and np.all(ref[flat][:, :2] == 0)
    assert np.array_equal(sfv.label_distance_sums(_dev(C), lab, S, "hamming").cpu().numpy(), ref)


def test_sums_refused_shapes_write_nothing():
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")       # noqa: E731
    zi = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")        # noqa: E731
    for entry, dtype in (("rbvae_label_dist_sums", torch.float64), ("rbvae_label_hamming_sums", torch.int32)):
        sums = Guarded(dtype, 4, 2)
        for N, Ld, S, match in ((4, 129, 2, "L=129"), (0, 3, 2, "N=0"), (16385, 3, 2, "N=16385"), (4, 3, 0, "S=0"),
                                (4, 3, 257, "S=257")):
            assert sfv._lib.query("rbvae_label_sums_ok", N, Ld, S) == 0
            with pytest.raises(ValueError, match=match):
                sfv._lib.call(entry, z(4, 129), N, Ld, zi(4), zi(258), S, sums.t)
        with pytest.raises(ValueError, match="null"):
            sfv._lib.call(entry, z(4, 3), 4, 3, None, zi(3), 2, sums.t)
        sums.check(entry, untouched=True)


# ---- end to end ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["", "_edge"])
@pytest.mark.parametrize("metric", ["euclidean", "hamming"])
def test_silhouette_against_sklearn(gold, metric, which):
    lab = gold["lab" + which]
    ref = gold[("sil_euclid" if metric == "euclidean" else "sil_hamming") + which]
    s = sfv.silhouette_samples(_dev(gold["X"]), lab, metric=metric)
    d = np.abs(s - ref).max()
    print(f"silhouette ({metric}{which}): mean {s.mean():.6f}, max |device - sklearn| {d:.3g}")
    assert s.dtype == np.float64 and s.shape == (320,) and d <= 1e-12
    assert sfv.silhouette_score(_dev(gold["X"]), torch.from_numpy(lab).cuda(), metric=metric) == float(np.mean(s))
    if which:
        assert s[0] == 0.0


@pytest.mark.parametrize("k", [5, 24])
def test_knn_label_agreement_against_sklearn(gold, k):
    out = sfv.knn_label_agreement(_dev(gold["X"]), gold["lab"], k)
    assert out["purity"] == float(gold[f"purity_{k}"]) and out["accuracy"] == float(gold[f"acc_{k}"])
    assert out["predictions"].dtype == np.int64 and np.array_equal(out["predictions"], gold[f"pred_{k}"])
    wide = sfv.knn_label_agreement(_dev(gold["X"]), gold["lab"], k, n_states=12)
    assert np.array_equal(wide["predictions"], out["predictions"])


def test_latent_scores():
    F_, RES, LD = 40, 64, 16
    torch.manual_seed(0)
    model = sfv.Seq2SeqBinaryVAE(3, 3, LD, LD, variant="contrastive", input_hw=(RES, RES), compute_dtype="f32").cuda().eval()
    x = torch.rand(F_, 3, RES, RES, generator=torch.Generator().manual_seed(1)).cuda()
    u = torch.rand(F_, LD, generator=torch.Generator().manual_seed(2))
    flags = [10, 30]
    out = sfv.latent_scores(model, x, range(F_), flags, n_neighbors=5, u=u)
    z = model.encode(x[:, None], temperature=0.2, hard=False, noise_ratio=0.3, u=u.cuda())[:, 0]
    c = model.encode(x[:, None], temperature=0.2, hard=True, noise_ratio=0.3, u=u.cuda())[:, 0]
    assert torch.equal(out["latents"], z) and torch.equal(out["codes"], c) and set(c.unique().tolist()) <= {0.0, 1.0}
    assert np.array_equal(out["labels"], [sfv.assign_label(f, flags) for f in range(F_)])
    names = ["silhouette", "silhouette_hamming", "knn_purity", "knn_accuracy"]
    assert all(np.isfinite(out[n]) for n in names) and "trustworthiness_pca" not in out
    assert out["silhouette"] == sfv.silhouette_score(out["latents"], out["labels"], 3)
    assert out["silhouette_hamming"] == sfv.silhouette_score(out["codes"], out["labels"], 3, metric="hamming")
    assert out["knn_purity"] == sfv.knn_label_agreement(out["latents"], out["labels"], 5, 3)["purity"]
    assert -1.0 <= out["silhouette"] <= 1.0 and 0.0 <= out["knn_accuracy"] <= 1.0 and not model.training
    proj = sfv.latent_projections(model, x, u=u, frame_indices=range(F_), flags=flags, perplexity=5.0, max_iter=250)
    both = sfv.latent_scores(model, x, range(F_), flags, projections=proj, n_neighbors=5, u=u)
    assert both["latents"] is proj["latents"] or torch.equal(both["latents"], proj["latents"])
    assert all(both[n] == out[n] for n in names)
    for name in ("pca", "tsne"):
        Y = proj[name].embedding.float().contiguous()
        assert both[f"trustworthiness_{name}"] == sfv.trustworthiness(z, Y, 5)
        assert both[f"continuity_{name}"] == sfv.trustworthiness(Y, z, 5)
        assert 0.0 <= both[f"trustworthiness_{name}"] <= 1.0 and 0.0 <= both[f"continuity_{name}"] <= 1.0


def test_invalid_arguments(gold):
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")       # noqa: E731
    lab = np.array([0, 0, 0, 0, 1, 1, 1, 1])
    nbr = torch.zeros((8, 3), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="GPU"):
        sfv.neighbour_ranks(z(8, 3).cpu(), nbr)
    with pytest.raises(ValueError, match="GPU"):
        sfv.neighbour_ranks(z(8, 3), nbr.cpu())
    with pytest.raises(ValueError, match="int32"):
        sfv.neighbour_ranks(z(8, 3), nbr.long())
    with pytest.raises(ValueError, match="float32"):
        sfv.neighbour_ranks(z(8, 3).double(), nbr)
    with pytest.raises(ValueError, match="rows"):
        sfv.neighbour_ranks(z(9, 3), nbr)
    with pytest.raises(ValueError, match="k=8"):
        sfv.neighbour_ranks(z(8, 3), torch.zeros((8, 8), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="float32"):
        sfv.trustworthiness(z(8, 3), z(8, 2).double(), 3)   # the PCA's f64 embedding is converted by the caller
    with pytest.raises(ValueError, match="GPU"):
        sfv.trustworthiness(z(8, 3), z(8, 2).cpu(), 3)
    with pytest.raises(ValueError, match="rows"):
        sfv.trustworthiness(z(8, 3), z(7, 2), 3)
    for k in (4, 5, 0):                                     # scikit-learn: n_neighbors < n_samples / 2
        with pytest.raises(ValueError, match="n_neighbors"):
            sfv.trustworthiness(z(8, 3), z(8, 2), k)
    bad = z(8, 3)
    bad[2, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        sfv.trustworthiness(bad, z(8, 2), 3)
    with pytest.raises(ValueError, match="NaN"):
        sfv.silhouette_samples(bad, lab)
    with pytest.raises(ValueError, match="metric"):
        sfv.label_distance_sums(z(8, 3), lab, 2, metric="cosine")
    with pytest.raises(ValueError, match="labels"):
        sfv.label_distance_sums(z(8, 3), lab[:7], 2)
    with pytest.raises(ValueError, match="labels"):
        sfv.label_distance_sums(z(8, 3), lab.astype(np.float32), 2)
    with pytest.raises(ValueError, match="labels outside"):
        sfv.label_distance_sums(z(8, 3), lab, 1)
    with pytest.raises(ValueError, match="labels outside"):
        sfv.label_distance_sums(z(8, 3), lab - 1, 2)
    with pytest.raises(ValueError, match="S=257"):
        sfv.label_distance_sums(z(8, 3), lab, 257)
    with pytest.raises(ValueError, match="float32"):
        sfv.silhouette_samples(z(8, 3).double(), lab)
    with pytest.raises(ValueError, match="Number of labels is 1"):
        sfv.silhouette_samples(z(8, 3), np.zeros(8, dtype=np.int64), 4)
    with pytest.raises(ValueError, match="Number of labels is 8"):
        sfv.silhouette_samples(z(8, 3), np.arange(8))
    with pytest.raises(ValueError, match="k=8"):
        sfv.knn_label_agreement(z(8, 3), lab, 8)
    with pytest.raises(ValueError, match="frame indices"):
        sfv.latent_scores(None, z(2, 3, 8, 8), [0], [1])
    with pytest.raises(ValueError, match="F, C, H, W"):
        sfv.latent_scores(None, z(2, 3, 8), [0, 1], [1])
