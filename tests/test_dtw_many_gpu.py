"""GPU: many sequences aligned on the device (the batched entries of csrc/dtw.hip, alignment.py) against tests/_dtw_many_ref.py
and against the single-pair entries run on the same device.  Every comparison is exact: for every pair of a batch the packed
directions, the last row, the path, the state and the cost are the restatement's and the single-pair entries' bits, whatever else
is in the batch; lo, hi, count and the updated template of the DBA step, every inertia, the returned template and its paths are
the restatement's bits.  Every output sits in sentinel guard bands, and the padding between the dirs blocks is never written.
The stack has sequences of 1, 2, TI - 1, TI, TI + 1 and 2 TI + 2 rows, so the pairs of a batch differ in launch count, some are
finished many launches before the batch ends, and one pair has more tiles on a diagonal than the others; test_dtw_many_cpu.py
shows that each named defect of the restatement changes a result on these same cases.

Measured on one MI355X: every comparison exact on the first run; the 31 tests take 3.5 s together, none more than 0.4 s.
"""
import numpy as np
import pytest
import torch

import _dtw_many_ref as MR
import _dtw_ref as R
import sfv_amd as sfv

pytestmark = pytest.mark.gpu

q = sfv._lib.query
call = sfv._lib.call
TI, TJ = q("rbvae_dtw_tile_rows"), q("rbvae_dtw_tile_cols")
TILE = (TI, TJ)
MET = {"sqeuclidean": 0, "euclidean": 1, "hamming": 2}
GUARD = 4096
SENT = {torch.float64: (torch.int64, 0x7FF8DEADDEADBEEF), torch.int32: (torch.int32, -0x21524111), torch.uint8: (torch.uint8, 0xA5),
        torch.int64: (torch.int64, -0x2152411021524111), torch.float32: (torch.int32, 0x7FC0BEEF)}


class Guarded:
    """n elements of dtype inside GUARD sentinel elements on each side (a NaN sentinel for the floats)"""

    def __init__(self, dtype, *shape):
        self.n = int(np.prod(shape))
        raw, self.sent = SENT[dtype]
        self.buf = torch.full((GUARD + self.n + GUARD,), self.sent, dtype=raw, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.n].view(dtype).view(*shape)

    def check(self, what, untouched=False, full=True):
        bits = self.buf.cpu().numpy()
        inner = np.zeros(bits.shape, dtype=bool)
        inner[GUARD:GUARD + self.n] = True
        stray = np.nonzero((bits != self.sent) & ~inner)[0]
        assert stray.size == 0, f"{what}: {stray.size} elements outside the output were written; first at {stray[0] - GUARD}"
        unwritten = np.nonzero((bits == self.sent) & inner)[0]
        if untouched:
            assert unwritten.size == self.n, f"{what}: a refused call wrote {self.n - unwritten.size} elements"
        elif full:
            assert unwritten.size == 0, f"{what}: {unwritten.size} elements never written; first at {unwritten[0] - GUARD}"
        return self.t.cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the shared inputs are read-only


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else (a.view(np.int32) if a.dtype == np.float32 else a)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _plan(len_x, len_y, pairs):
    """rbvae_dtw_pairs_sizes and _plan -> (offsets, totals, guarded plan, (n_diag, max_tiles))"""
    lx, ly, pr = _i32(len_x), _i32(len_y), _i32(pairs).reshape(-1, 2)
    P = len(pr)
    off = {k: np.zeros(P + 1, dtype=np.int64) for k in ("dirs", "last", "ws", "path")}
    totals = np.zeros(4, dtype=np.uint64)
    rc = sfv._lib.lib().rbvae_dtw_pairs_sizes(lx.ctypes.data, len(lx), ly.ctypes.data, len(ly), pr.ctypes.data, P,
                                              *[o.ctypes.data for o in off.values()], totals.ctypes.data)
    assert rc == 0
    nbytes = q("rbvae_dtw_pairs_plan_bytes", P)
    plan = Guarded(torch.int64, nbytes // 8)
    launch = np.zeros(2, dtype=np.int32)
    call("rbvae_dtw_pairs_plan", lx.ctypes.data, len(lx), ly.ctypes.data, len(ly), pr.ctypes.data, P, plan.t, nbytes,
         launch.ctypes.data)
    assert tuple(launch) == MR.launch_numbers(lx, ly, pr, TILE)
    plan.check("plan")
    return off, [int(t) for t in totals], plan, (int(launch[0]), int(launch[1]))


def _raw_pairs(X, len_x, Y, len_y, pairs, metric):
    """the batched entries called directly on guarded buffers -> per pair what they wrote"""
    what = f"({len(pairs)} pairs, {X.shape[1]}, {metric})"
    off, (nd, nl, nw, npath), plan, (n_diag, max_tiles) = _plan(len_x, len_y, pairs)
    P, Ld = len(pairs), X.shape[1]
    dirs, last, ws = Guarded(torch.uint8, nd), Guarded(torch.float64, nl), Guarded(torch.float64, nw // 8)
    path, state, cost = Guarded(torch.int32, npath, 2), Guarded(torch.int32, P, 3), Guarded(torch.float64, P)
    Xd, Yd = _dev(X), _dev(Y)
    tail = (plan.t, P, n_diag, max_tiles, dirs.t, nd, last.t, nl, ws.t, nw)
    if metric == "hamming":
        call("rbvae_dtw_pairs_fill_bits", sfv.pack_codes(Xd), len(X), sfv.pack_codes(Yd), len(Y), Ld, *tail)
    else:
        call("rbvae_dtw_pairs_fill", Xd, len(X), Yd, len(Y), Ld, MET[metric], *tail)
    call("rbvae_dtw_pairs_trace", dirs.t, nd, last.t, nl, plan.t, P, path.t, npath, state.t, cost.t)
    ws.check("workspace " + what, full=False)
    plan.check("plan " + what)
    d, lr, pa = dirs.check("dirs " + what, full=False), last.check("last_row " + what), path.check("path " + what, full=False)
    st, co = state.check("state " + what), cost.check("cost " + what)
    out = []
    for p, (a, b) in enumerate(pairs):
        n, m = int(len_x[a]), int(len_y[b])
        W4 = (m + 3) // 4
        d0, d1 = int(off["dirs"][p]), int(off["dirs"][p + 1])
        assert np.all(d[d0 + n * W4:d1] == 0xA5), f"{what}: the padding behind the dirs block of pair {p} was written"
        ln = int(st[p, 0])
        assert 1 <= ln <= n + m - 1, f"{what}: pair {p} has len = {ln}"
        r0 = int(off["path"][p])
        out.append({"packed": d[d0:d0 + n * W4].reshape(n, W4), "last_row": lr[int(off["last"][p]):int(off["last"][p + 1])],
                    "path": pa[r0:r0 + ln].astype(np.int64), "cost": float(co[p]), "start": int(st[p, 1]), "end": int(st[p, 2])})
    return out


def _single(x, y, metric):
    """the single-pair entries on the same device"""
    (n, Ld), m = x.shape, len(y)
    dirs = torch.empty(q("rbvae_dtw_dirs_bytes", n, m), dtype=torch.uint8, device="cuda")
    last, ws = torch.empty(m, dtype=torch.float64, device="cuda"), torch.empty(q("rbvae_dtw_ws_bytes", n, m) // 8, dtype=torch.float64,
                                                                               device="cuda")
    xd, yd = _dev(x), _dev(y)
    if metric == "hamming":
        call("rbvae_dtw_fill_bits", sfv.pack_codes(xd), n, sfv.pack_codes(yd), m, Ld, -1, 0, dirs, last, None, ws)
    else:
        call("rbvae_dtw_fill", xd, n, yd, m, Ld, MET[metric], -1, 0, dirs, last, None, ws)
    path = torch.empty((n + m - 1, 2), dtype=torch.int32, device="cuda")
    state, cost = torch.empty(3, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.float64, device="cuda")
    call("rbvae_dtw_trace", dirs, last, n, m, 0, path, state, cost)
    ln, start, end = state.cpu().tolist()
    return {"packed": dirs.cpu().numpy().reshape(n, (m + 3) // 4), "last_row": last.cpu().numpy(),
            "path": path[:ln].cpu().numpy().astype(np.int64), "cost": float(cost.cpu()[0]), "start": start, "end": end}


def _pair_agrees(got, ref, what):
    ok = np.array_equal(got["packed"], ref["packed"]) and _same(got["last_row"], ref["last_row"])
    ok = ok and np.array_equal(got["path"], ref["path"]) and _same(np.array([got["cost"]]), np.array([ref["cost"]]))
    assert ok and (got["start"], got["end"]) == (ref["start"], ref["end"]), what


# ---- every pair of a batch, bit for bit ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("second", [False, True], ids=["all_pairs", "second_batch"])
@pytest.mark.parametrize("kind,L", MR.INPUTS)
def test_every_pair_is_the_single_pair_result(kind, L, second):
    lengths = MR.stack_lengths(TI)
    X = MR.make_stack(kind, L, lengths)
    seqs = MR.split(X, lengths)
    pairs = MR.SECOND_BATCH if second else MR.all_pairs(len(lengths))
    for metric in R.metrics_of(kind):
        got = _raw_pairs(X, lengths, X, lengths, pairs, metric)
        ref = MR.stack_reference(kind, L, metric, TI, TJ, second)
        again = _raw_pairs(X, lengths, X, lengths, pairs, metric)
        for p, (a, b) in enumerate(pairs):
            what = f"{kind} {L} {metric}: pair {p} = ({a}, {b})"
            _pair_agrees(got[p], ref[p], what + " against the restatement")
            _pair_agrees(got[p], _single(seqs[a], seqs[b], metric), what + " against the single-pair entries")
            _pair_agrees(again[p], got[p], what + ": two runs differ")
    if second:                                              # a repeated pair, and P = 1 with another stack on the Y side
        assert np.array_equal(got[3]["packed"], got[4]["packed"]) and np.array_equal(got[3]["path"], got[4]["path"])
        one = _raw_pairs(seqs[5], [lengths[5]], X, lengths, [(0, 2)], metric)
        _pair_agrees(one[0], _single(seqs[5], seqs[2], metric), "P = 1")


@pytest.mark.parametrize("kind,L,metric", [("repeat", 50, "euclidean"), ("code", 50, "hamming"), ("soft", 1, "sqeuclidean")])
def test_chunking_changes_nothing(kind, L, metric):
    lengths = MR.stack_lengths(TI)
    X = MR.make_stack(kind, L, lengths)
    Xd = _dev(X)
    ref = MR.stack_reference(kind, L, metric, TI, TJ, False)
    whole = sfv.dtw_pairs(Xd, lengths, metric=metric)
    sizes = [sfv.alignment._pair_bytes(lengths[a], lengths[b], TI, TJ) for a, b in MR.all_pairs(len(lengths))]
    for max_bytes in (1, max(sizes), 2 * max(sizes)):       # one pair a chunk; the largest pair alone; at most two of the large ones
        chunks = sfv.alignment._chunks(_i32(lengths), _i32(lengths), MR.all_pairs(len(lengths)), max_bytes)
        assert len(chunks) > 1 and sum(chunks, []) == MR.all_pairs(len(lengths)) and (max_bytes > 1 or len(chunks) == 15)
        assert all(len(c) == 1 or sum(sizes[MR.all_pairs(6).index(p)] for p in c) <= max_bytes for c in chunks)
        got = sfv.dtw_pairs(Xd, lengths, metric=metric, max_bytes=max_bytes)
        assert len(got) == len(whole) == 15
        for g, w, r, (a, b) in zip(got, whole, ref, MR.all_pairs(len(lengths))):
            assert isinstance(g, sfv.DTWResult) and g.path.dtype == np.int64 and g.table is None and g.last_row.is_cuda
            assert np.array_equal(g.path, w.path) and _same(np.array([g.cost, g.normalized_cost]), np.array([w.cost, w.normalized_cost]))
            assert torch.equal(g.last_row, w.last_row) and (g.start, g.end, g.path_len) == (0, lengths[b] - 1, len(r["path"]))
            assert np.array_equal(g.path, r["path"]) and _same(np.array([g.cost]), np.array([r["cost"]]))
            assert _same(g.last_row.cpu().numpy(), r["last_row"]) and g.normalized_cost == g.cost / g.path_len
    # the other order of every pair through a pair list: the cost has the same bits, as the contract says
    swapped = sfv.dtw_pairs(Xd, lengths, [(b, a) for a, b in MR.all_pairs(len(lengths))], metric=metric)
    assert all(_same(np.array([s.cost]), np.array([w.cost])) for s, w in zip(swapped, whole))
    # two stacks
    seqs = MR.split(X, lengths)
    two = sfv.dtw_pairs(_dev(seqs[4]), [lengths[4]], [(0, 5), (0, 2)], Y=Xd, lengths_y=lengths, metric=metric)
    assert np.array_equal(two[0].path, ref[MR.all_pairs(6).index((4, 5))]["path"])
    assert np.array_equal(two[1].path, R.dtw(seqs[4], seqs[2], metric, tile=TILE)["path"])


# ---- ranges and the update ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,T,lengths,L", MR.update_cases(TI), ids=[f"{c[0]}-{c[3]}" for c in MR.update_cases(TI)])
def test_path_ranges_and_update(name, T, lengths, L):
    tmpl, seqs, res, ranges, (new, count) = MR.update_case(T, lengths, L, TI, TJ)
    S = len(seqs)
    lo, hi = Guarded(torch.int32, S, T), Guarded(torch.int32, S, T)
    for s, (r, m) in enumerate(zip(res, lengths)):
        path = Guarded(torch.int32, T + m - 1, 2)           # as the trace leaves it: the path in front, scratch behind
        path.t[:len(r["path"])] = _dev(r["path"].astype(np.int32))
        state = _dev(np.array([len(r["path"]), 0, m - 1], dtype=np.int32))
        before = path.buf.clone()
        call("rbvae_dtw_path_ranges", path.t, state, T, m, lo.t[s], hi.t[s])
        assert torch.equal(path.buf, before)
    glo, ghi = lo.check("lo"), hi.check("hi")
    for s, (rlo, rhi) in enumerate(ranges):
        assert np.array_equal(glo[s], rlo) and np.array_equal(ghi[s], rhi), f"sequence {s}"
    _, _, plan, _ = _plan([T], lengths, [(0, s) for s in range(S)])
    Y = _dev(np.concatenate(seqs))
    out, cnt = Guarded(torch.float32, T, L), Guarded(torch.int32, T)
    call("rbvae_dtw_barycenter_update", Y, len(Y), L, plan.t, S, lo.t, hi.t, T, out.t, cnt.t)
    assert _same(out.check("template"), new) and np.array_equal(cnt.check("count"), count)
    lo.check("lo")
    hi.check("hi")
    # no path: nothing is written
    none = Guarded(torch.int32, T)
    call("rbvae_dtw_path_ranges", path.t, _dev(np.array([-1, -1, 0], dtype=np.int32)), T, lengths[-1], none.t, none.t)
    none.check("lo of no path", untouched=True)


# ---- the whole iteration ----------------------------------------------------------------------------------------------------------------------

def _barycenter_agrees(got, ref, S):
    assert isinstance(got, sfv.DTWBarycenter) and got.template.is_cuda and got.template.dtype == torch.float32
    assert len(got.inertia) == len(ref["inertia"]) and _same(np.array(got.inertia), np.array(ref["inertia"])), (got.inertia, ref["inertia"])
    assert (got.n_iter, got.reason, got.converged) == (ref["n_iter"], ref["reason"], ref["reason"] == "converged")
    assert _same(got.template.cpu().numpy(), ref["template"])
    assert got.count.dtype == torch.int32 and np.array_equal(got.count.cpu().numpy(), ref["count"])
    assert len(got.results) == S
    for r, p, c in zip(got.results, ref["paths"], ref["costs"]):
        assert np.array_equal(r.path, p) and _same(np.array([r.cost]), np.array([c]))


@pytest.mark.parametrize("init,max_iter", MR.DBA_RUNS)
def test_barycenter(init, max_iter):
    c = MR.DBA_CASE
    base, copies, _, _ = MR.planted(c["S"], c["n"], c["L"], c["seed"])
    lengths = [len(y) for y in copies]
    assert min(lengths) > 2 * TI and max(lengths) <= 4 * TI
    ref = MR.dba_reference(init, TI, TJ, max_iter)
    X = _dev(np.concatenate(copies))
    got = sfv.dtw_barycenter(X, lengths, init=_dev(base) if init == "tensor" else init, max_iter=max_iter, tol=c["tol"])
    _barycenter_agrees(got, ref, c["S"])
    assert ref["n_iter"] >= 2 and (max_iter != 2 or ref["reason"] == "max_iter")
    if init == 0:                                           # chunks of one pair: the same bits
        _barycenter_agrees(sfv.dtw_barycenter(X, lengths, init=0, max_iter=max_iter, tol=c["tol"], max_bytes=1), ref, c["S"])


def test_barycenter_fixed_points():
    y = np.array(MR.make_stack("soft", 3, (TI + 5,)))
    got = sfv.dtw_barycenter(_dev(np.concatenate([y] * 3)), [len(y)] * 3, init=1)
    assert got.inertia == [0.0, 0.0] and (got.n_iter, got.reason) == (1, "converged") and _same(got.template.cpu().numpy(), y)
    assert np.all(got.count.cpu().numpy() == 3)
    zero = sfv.dtw_barycenter(_dev(np.concatenate([y] * 2)), [len(y)] * 2, init=0, max_iter=0)
    assert (zero.n_iter, zero.reason, zero.inertia) == (0, "max_iter", [0.0])


# ---- the matrix, the medoid, the votes ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,L,metric", [("soft", 50, "sqeuclidean"), ("code", 50, "hamming")])
def test_distance_matrix_and_medoid(kind, L, metric):
    lengths = MR.stack_lengths(TI)
    X = MR.make_stack(kind, L, lengths)
    ref = MR.distance_matrix(MR.split(X, lengths), metric, TILE)
    got = sfv.dtw_distance_matrix(_dev(X), lengths, metric=metric, max_bytes=1 << 16)
    assert _same(got["cost"], ref["cost"]) and got["path_len"].dtype == np.int64 and np.array_equal(got["path_len"], ref["path_len"])
    assert _same(got["normalized"], ref["normalized"]) and np.array_equal(got["cost"], got["cost"].T)
    assert np.all(np.diag(got["cost"]) == 0) and np.diag(got["path_len"]).tolist() == list(lengths)
    assert sorted(got["results"]) == MR.all_pairs(len(lengths))
    assert all(np.array_equal(got["results"][k].path, ref["results"][k]["path"]) for k in ref["results"])
    gm, rm = sfv.dtw_medoid(got["cost"]), MR.medoid(ref["cost"])
    assert gm["index"] == rm["index"] and _same(gm["total"], rm["total"]) and _same(gm["mean_to_others"], rm["mean_to_others"])
    assert sfv.dtw_medoid(MR.MEDOID_TIE)["index"] == MR.medoid(MR.MEDOID_TIE)["index"] == 0
    v = MR.VOTE_CASE
    carried = [sfv.transfer_labels(p, la, v["M"]) for p, la in zip(v["paths"], v["labels"])]
    assert np.array_equal(sfv.vote_labels(carried), MR.vote(v["paths"], v["labels"], v["M"], v["K"]))
    one = sfv.dtw_distance_matrix(_dev(X[:5]), [5], metric=metric)
    assert one["cost"].tolist() == [[0.0]] and one["path_len"].tolist() == [[5]] and one["results"] == {}


# ---- latent_alignment_videos ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("holdout", [None, 1])
def test_latent_alignment_videos(holdout):
    hw, LD = (16, 24), 32
    torch.manual_seed(0)
    model = sfv.Seq2SeqBinaryVAE(4, 4, LD, LD, variant="percep", input_hw=hw, compute_dtype="f32").cuda().eval()
    case = MR.videos_case()
    V = len(case)
    g = torch.Generator().manual_seed(1)
    videos = [torch.randn(len(y), 4, *hw, generator=g).cuda() for y, _, _, _ in case]
    u = [torch.rand(len(y), LD, generator=g) for y, _, _, _ in case]
    lat = [_dev(y) for y, _, _, _ in case]
    out = sfv.latent_alignment_videos(model, videos, [c[2] for c in case], [c[3] for c in case], holdout, latents=lat, u=u,
                                      max_iter=4)
    assert set(out) == {"latents", "codes", "labels", "lengths", "soft", "hard", "medoid", "outlier_scores", "fitted", "barycenter",
                        "paths", "warp", "template_labels", "transfers"}
    labels, lengths = [c[1] for c in case], [len(c[0]) for c in case]
    assert all(np.array_equal(a, b) for a, b in zip(out["labels"], labels)) and out["lengths"] == lengths
    assert all(torch.equal(a, b) for a, b in zip(out["latents"], lat))
    codes = [model.encode(x[:, None], temperature=0.2, hard=True, noise_ratio=0.3, u=uu.cuda())[:, 0].float() for x, uu in zip(videos, u)]
    assert all(torch.equal(a, b) for a, b in zip(out["codes"], codes))
    z = [c[0] for c in case]
    soft, hard = MR.distance_matrix(z, "sqeuclidean", TILE), MR.distance_matrix([c.cpu().numpy() for c in codes], "hamming", TILE)
    assert _same(out["soft"]["cost"], soft["cost"]) and _same(out["hard"]["cost"], hard["cost"])
    assert out["medoid"]["soft"]["index"] == MR.medoid(soft["cost"])["index"]
    assert out["medoid"]["hard"]["index"] == MR.medoid(hard["cost"])["index"]
    assert _same(out["outlier_scores"], MR.medoid(soft["cost"])["mean_to_others"])
    fitted = [v for v in range(V) if v != holdout]
    assert out["fitted"] == fitted
    bary = MR.barycenter([z[v] for v in fitted], "medoid", 4, 1e-6, TILE)
    _barycenter_agrees(out["barycenter"], bary, len(fitted))
    T, K = len(bary["template"]), 3
    paths = dict(zip(fitted, bary["paths"]))
    if holdout is not None:
        paths[holdout] = R.dtw(bary["template"], z[holdout], "sqeuclidean", tile=TILE)["path"]
    for v in range(V):
        assert np.array_equal(out["paths"][v], paths[v])
        wm = sfv.warp_map(paths[v], T, lengths[v])
        assert all(np.array_equal(out["warp"][v][k], wm[k]) for k in wm)
    assert sorted(out["transfers"]) == ([holdout] if holdout is not None else list(range(V)))
    for t, got in out["transfers"].items():
        others = [v for v in range(V) if v != t]
        to_t = {a: soft["results"][(a, t)]["path"] if a < t else soft["results"][(t, a)]["path"][:, ::-1] for a in others}
        near = min(others, key=lambda a: (soft["cost"][t, a], a))
        sources = [s for s in fitted if s != t]
        tl = MR.vote([paths[s][:, ::-1] for s in sources], [labels[s] for s in sources], T, K)
        want = {"nearest": MR.transfer(to_t[near], labels[near], lengths[t], K),
                "vote": MR.vote([to_t[a] for a in others], [labels[a] for a in others], lengths[t], K),
                "barycenter": MR.transfer(paths[t], tl, lengths[t], K)}
        assert got["nearest"]["source"] == near
        true_t = np.nonzero(labels[t][1:] != labels[t][:-1])[0] + 1
        for way, w in want.items():
            g = got[way]
            assert g["labels"].dtype == np.int64 and np.array_equal(g["labels"], w), (t, way)
            assert g["accuracy"] == float((w == labels[t]).mean())
            bounds = np.nonzero(w[1:] != w[:-1])[0] + 1
            assert np.array_equal(g["boundaries"], bounds)
            ba = sfv.boundary_agreement(bounds, true_t, 2)
            assert g["boundary_agreement"].keys() == ba.keys()
            assert all(g["boundary_agreement"][k] == ba[k] or ba[k] != ba[k] for k in ba)
            agree = sfv.clustering_agreement(labels[t], torch.from_numpy(w).cuda(), K, K)
            assert g["label_agreement"]["ari"] == agree["ari"]
    assert np.array_equal(out["template_labels"], MR.vote([paths[s][:, ::-1] for s in fitted], [labels[s] for s in fitted], T, K))


# ---- refused without a launch and without a write ---------------------------------------------------------------------------------------

def test_refused_arguments_write_nothing():
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")           # noqa: E731
    plan, dirs, last, ws = Guarded(torch.int64, 64), Guarded(torch.uint8, 4096), Guarded(torch.float64, 256), Guarded(torch.float64, 1024)
    path, state, cost = Guarded(torch.int32, 512, 2), Guarded(torch.int32, 4, 3), Guarded(torch.float64, 4)
    lo, out, cnt = Guarded(torch.int32, 64), Guarded(torch.float32, 64, 3), Guarded(torch.int32, 64)
    launch = np.full(2, -7, dtype=np.int32)
    err = sfv._lib.lib().rbvae_last_error
    for lx, ly, pr, P, match in (([5, 0], [5, 7], [(0, 1)], 1, "len_x\\[1\\]=0"), ([5, 7], [16385], [(0, 0)], 1, "len_y\\[0\\]=16385"),
                                 ([5, 7], [5, 7], [(2, 0)], 1, "pairs\\[0\\]\\[0\\]=2"), ([5, 7], [5, 7], [(0, 2)], 1, "pairs\\[0\\]\\[1\\]=2"),
                                 ([5, 7], [5, 7], [(0, 1)], 0, "P=0")):
        a, b, c = _i32(lx), _i32(ly), _i32(pr)
        with pytest.raises(RuntimeError, match=match):
            call("rbvae_dtw_pairs_plan", a.ctypes.data, len(a), b.ctypes.data, len(b), c.ctypes.data, P, plan.t, 8 * 64,
                 launch.ctypes.data)
        assert b"dtw_pairs_plan" in err()
    a = _i32([5, 7])
    with pytest.raises(ValueError, match="needed"):         # a plan too small
        call("rbvae_dtw_pairs_plan", a.ctypes.data, 2, a.ctypes.data, 2, _i32([(0, 1)]).ctypes.data, 1, plan.t, 8, launch.ctypes.data)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_dtw_pairs_plan", a.ctypes.data, 2, a.ctypes.data, 2, _i32([(0, 1)]).ctypes.data, 1, None, 8 * 64, launch.ctypes.data)
    assert np.all(launch == -7)
    X, B = z(12, 129), torch.zeros((12, 4), dtype=torch.int32, device="cuda")
    good = sfv.alignment._PairBatch(a, a, [(0, 1)], "cuda")
    tail = (dirs.t, 4096, last.t, 256, ws.t, 8 * 1024)
    # (Nx, Ny, L, metric, P, n_diag, max_tiles) and what the message names
    for Nx, Ny, Ld, met, P, nd, mt, match in ((12, 12, 129, 0, 1, 1, 1, "L=129"), (12, 12, 0, 0, 1, 1, 1, "L=0"), (12, 12, 3, 3, 1, 1, 1, "metric=3"),
                                              (0, 12, 3, 0, 1, 1, 1, "Nx=0"), (12, 12, 3, 0, 0, 1, 1, "P=0"), (12, 12, 3, 0, 65536, 1, 1, "P=65536"),
                                              (12, 12, 3, 0, 1, 0, 1, "n_diag=0"), (12, 12, 3, 0, 1, 512, 1, "n_diag=512"),
                                              (12, 12, 3, 0, 1, 1, 257, "max_tiles=257")):
        with pytest.raises(RuntimeError, match=match):
            call("rbvae_dtw_pairs_fill", X, Nx, X, Ny, Ld, met, good.plan, P, nd, mt, *tail)
        if met != 3:
            with pytest.raises(RuntimeError, match=match):
                call("rbvae_dtw_pairs_fill_bits", B, Nx, B, Ny, Ld, good.plan, P, nd, mt, *tail)
    with pytest.raises(RuntimeError, match="fill_bits"):    # packed codes have their own entry
        call("rbvae_dtw_pairs_fill", X, 12, X, 12, 3, 2, good.plan, 1, 1, 1, *tail)
    for bad in range(4):
        args = [X, 12, X, 12, 3, 0, good.plan, 1, 1, 1, dirs.t, 4096, last.t, 256, ws.t, 8 * 1024]
        args[(0, 6, 10, 14)[bad]] = None
        with pytest.raises(ValueError, match="null"):
            call("rbvae_dtw_pairs_fill", *args)
    for P in (0, 65536):
        with pytest.raises(RuntimeError, match=f"P={P}"):
            call("rbvae_dtw_pairs_trace", dirs.t, 4096, last.t, 256, good.plan, P, path.t, 512, state.t, cost.t)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_dtw_pairs_trace", dirs.t, 4096, last.t, 256, good.plan, 1, path.t, 512, state.t, None)
    for n, m, match in ((0, 5, "n=0"), (5, 16385, "m=16385")):
        with pytest.raises(RuntimeError, match=match):
            call("rbvae_dtw_path_ranges", path.t, state.t, n, m, lo.t, lo.t)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_dtw_path_ranges", path.t, None, 5, 5, lo.t, lo.t)
    for Ny, Ld, P, T, match in ((0, 3, 1, 5, "Ny=0"), (12, 129, 1, 5, "L=129"), (12, 3, 0, 5, "P=0"), (12, 3, 1, 0, "T=0"),
                                (12, 3, 1, 16385, "T=16385")):
        with pytest.raises(RuntimeError, match=match):
            call("rbvae_dtw_barycenter_update", X, Ny, Ld, good.plan, P, lo.t, lo.t, T, out.t, cnt.t)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_dtw_barycenter_update", X, 12, 3, good.plan, 1, lo.t, lo.t, 5, None, cnt.t)
    for gd, what in ((plan, "plan"), (dirs, "dirs"), (last, "last_row"), (ws, "workspace"), (path, "path"), (state, "state"),
                     (cost, "cost"), (lo, "lo"), (out, "template"), (cnt, "count")):
        gd.check(what, untouched=True)
    bad = z(12, 3)
    bad[2, 1] = float("nan")
    for fn, match in ((lambda: sfv.dtw_pairs(z(12, 3).cpu(), [5, 7]), "GPU"), (lambda: sfv.dtw_pairs(bad, [5, 7]), "NaN"),
                      (lambda: sfv.dtw_pairs(z(12, 3), [5, 6]), "add to 11"), (lambda: sfv.dtw_pairs(z(12, 3), [12, 0]), "outside"),
                      (lambda: sfv.dtw_pairs(z(12, 3), [5, 7], [(0, 2)]), "names no sequence"),
                      (lambda: sfv.dtw_pairs(z(12, 3), [5, 7], Y=z(4, 5), lengths_y=[4], pairs=[(0, 0)]), "L=3.*L=5"),
                      (lambda: sfv.dtw_pairs(z(12, 3), [5, 7], Y=z(4, 3)), "come together"),
                      (lambda: sfv.dtw_pairs(z(12, 3), [5, 7], Y=z(4, 3), lengths_y=[4]), "pair list"),
                      (lambda: sfv.dtw_pairs(z(12, 129), [5, 7]), "outside"), (lambda: sfv.dtw_pairs(z(12, 3), [5, 7], metric="cosine"), "metric"),
                      (lambda: sfv.dtw_pairs(z(20000, 1), [20000]), "outside"),
                      (lambda: sfv.dtw_barycenter(z(12, 3), [5, 7], init=2), "init=2"), (lambda: sfv.dtw_barycenter(z(12, 3), [5, 7], init="mean"), "init"),
                      (lambda: sfv.dtw_barycenter(z(12, 3), [5, 7], init=z(4, 2)), "init is"),
                      (lambda: sfv.dtw_barycenter(z(12, 3), [5, 7], max_iter=-1), "max_iter"),
                      (lambda: sfv.latent_alignment_videos(None, [z(2, 3)], [[0]], [[1]]), "at least two"),
                      (lambda: sfv.latent_alignment_videos(None, [z(2, 3)] * 2, [[0]] * 2, [[1]] * 2, holdout=1), "holdout")):
        with pytest.raises(ValueError, match=match):
            fn()
    assert sfv.dtw_pairs(z(12, 3), [12]) == []
