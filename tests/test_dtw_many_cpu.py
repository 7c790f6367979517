"""CPU: tests/_dtw_many_ref.py (the restatement the GPU tests compare the many-sequence entries of csrc/dtw.hip with) tied down
without a device -- its launch-by-launch batched fill against _dtw_ref's plain loop, the range form of the update against a
cell-by-cell accumulation, the fixed points and the descent of DBA, planted data -- the named defects on the GPU test's own
cases, the host functions dtw_medoid and vote_labels, and the answers of rbvae_dtw_pairs_ok / _sizes / _plan_bytes, which need
the library but no GPU.
"""
import ctypes
import math

import numpy as np
import pytest

import _dtw_many_ref as MR
import _dtw_ref as R
import sfv_amd as sfv

q = sfv._lib.query
TI, TJ = q("rbvae_dtw_tile_rows"), q("rbvae_dtw_tile_cols")
TILE = (TI, TJ)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


# ---- the library's answers ------------------------------------------------------------------------------------------------------------

def _sizes(len_x, len_y, pairs, P=None):
    lx, ly, pr = _i32(len_x), _i32(len_y), _i32(pairs).reshape(-1, 2)
    P = len(pr) if P is None else P
    off = [np.full(max(P, 0) + 1, -7, dtype=np.int64) for _ in range(4)]
    totals = np.full(4, 12345, dtype=np.uint64)
    rc = sfv._lib.lib().rbvae_dtw_pairs_sizes(lx.ctypes.data, len(lx), ly.ctypes.data, len(ly), pr.ctypes.data, P,
                                              *[o.ctypes.data for o in off], totals.ctypes.data)
    return rc, off, totals


def _ok(len_x, len_y, pairs, L=3, metric=0, P=None):
    lx, ly, pr = _i32(len_x), _i32(len_y), _i32(pairs).reshape(-1, 2)
    return q("rbvae_dtw_pairs_ok", lx.ctypes.data, len(lx), ly.ctypes.data, len(ly), pr.ctypes.data, len(pr) if P is None else P,
             L, metric)


def test_sizes_are_the_single_pair_blocks_in_pair_order():
    assert q("rbvae_version") >= 111
    lengths = MR.stack_lengths(TI) + (16384, 12298)
    for pairs in (MR.all_pairs(len(lengths)), MR.SECOND_BATCH, [(7, 6)]):
        rc, (d, l, w, p), totals = _sizes(lengths, lengths, pairs)
        assert rc == 0 and _ok(lengths, lengths, pairs) == 1
        ref = MR.layout(lengths, lengths, pairs, TILE)
        assert np.array_equal(d, ref["dirs"]) and np.array_equal(l, ref["last"]) and np.array_equal(w, ref["ws"])
        assert np.array_equal(p, ref["path"]) and totals.tolist() == [d[-1], l[-1], w[-1], p[-1]]
        for k, (a, b) in enumerate(pairs):
            n, m = lengths[a], lengths[b]
            assert d[k] % 16 == 0 and 0 <= d[k + 1] - d[k] - q("rbvae_dtw_dirs_bytes", n, m) < 16
            assert w[k + 1] - w[k] == q("rbvae_dtw_ws_bytes", n, m) and l[k + 1] - l[k] == m and p[k + 1] - p[k] == n + m - 1
    # two stacks: a counts the X stack, b the Y stack
    rc, (d, l, w, p), _ = _sizes([5], [3, 9], [(0, 1), (0, 0)])
    assert rc == 0 and l.tolist() == [0, 9, 12] and p.tolist() == [0, 13, 20] and d.tolist() == [0, 16, 32]
    assert q("rbvae_dtw_pairs_plan_bytes", 1) == 8 * 14 and q("rbvae_dtw_pairs_plan_bytes", 65535) == 8 * (4 + 655350)
    assert q("rbvae_dtw_pairs_plan_bytes", 0) == 0 and q("rbvae_dtw_pairs_plan_bytes", 65536) == 0


def test_refusals_without_a_gpu():
    good = ([5, 7], [5, 7], [(0, 1)])
    assert _ok(*good) == 1 and _ok(*good, L=128, metric=2) == 1 and _ok([16384], [1], [(0, 0)]) == 1
    plan = np.full(64, -7, dtype=np.int64)
    launch = np.full(2, -7, dtype=np.int32)
    lib = sfv._lib.lib()
    for lx, ly, pr, P, match in (([5, 0], [5, 7], [(0, 1)], None, b"len_x[1]=0"), ([5, 7], [16385], [(0, 0)], None, b"len_y[0]=16385"),
                                 ([5, 7], [5, 7], [(2, 0)], None, b"pairs[0][0]=2"), ([5, 7], [5, 7], [(0, -1)], None, b"pairs[0][1]=-1"),
                                 ([5, 7], [5, 7], [(0, 1)], 0, b"P=0"), ([5, 7], [5, 7], [(0, 1)], 65536, b"P=65536")):
        assert _ok(lx, ly, pr, P=P) == 0
        rc, off, totals = _sizes(lx, ly, pr, P=P)
        assert rc == sfv._lib.E_UNSUPPORTED and match in lib.rbvae_last_error(), lib.rbvae_last_error()
        assert all(np.all(o == -7) for o in off) and np.all(totals == 12345)
        a, b, c = _i32(lx), _i32(ly), _i32(pr)
        rc = lib.rbvae_dtw_pairs_plan(a.ctypes.data, len(a), b.ctypes.data, len(b), c.ctypes.data, len(c) if P is None else P,
                                      plan.ctypes.data, plan.nbytes, launch.ctypes.data, None)
        assert rc == sfv._lib.E_UNSUPPORTED and np.all(plan == -7) and np.all(launch == -7)
    assert _ok(*good, L=129) == 0 and _ok(*good, L=0) == 0 and _ok(*good, metric=3) == 0 and _ok(*good, metric=-1) == 0
    a = _i32([5, 7])
    assert q("rbvae_dtw_pairs_ok", None, 2, a.ctypes.data, 2, a.ctypes.data, 1, 3, 0) == 0
    assert lib.rbvae_dtw_pairs_sizes(a.ctypes.data, 2, a.ctypes.data, 2, None, 1, None, None, None, None, None) == sfv._lib.E_INVALID


# ---- the restatement tied down ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", [(4, 8), TILE])
def test_batched_fill_is_the_plain_loop(tile):
    """launch by launch with every pair's own frontiers and corners = _dtw_ref's loop over the cells, for pairs of different
    launch counts in one batch"""
    lengths = (1, 2, 3, 4, 5, 11) if tile != TILE else MR.stack_lengths(TI)
    for kind, L, metric in (("soft", 3, "sqeuclidean"), ("repeat", 2, "euclidean"), ("code", 32, "hamming")):
        X = MR.make_stack(kind, L, lengths, seed=1)
        seqs = MR.split(X, lengths)
        pairs = MR.all_pairs(len(lengths)) + MR.SECOND_BATCH if tile != TILE else [(5, 4), (2, 5), (0, 1)]
        costs = [R.cost_matrix(seqs[a], seqs[b], metric) for a, b in pairs]
        for got, c in zip(MR.fill_batch(costs, tile), costs):
            ref = R.dtw_from_cost(c, tile=tile)
            assert np.array_equal(_bits(got["D"]), _bits(ref["D"])) and np.array_equal(got["dirs"], ref["dirs"])


def test_range_form_of_the_update_is_the_cell_by_cell_mean():
    for _, T, lengths, L in MR.update_cases(TI):
        tmpl, seqs, res, ranges, (new, count) = MR.update_case(T, lengths, L, TI, TJ)
        cells, ccount = MR.update_by_cells(seqs, [r["path"] for r in res], T)
        assert np.array_equal(new.view(np.int32), cells.view(np.int32)) and np.array_equal(count, ccount)
        assert count.min() >= len(seqs) and count.sum() == sum(len(r["path"]) for r in res)
        for (lo, hi), r, m in zip(ranges, res, lengths):
            wm = sfv.warp_map(r["path"], T, m)
            assert np.array_equal(lo, wm["first_j"]) and np.array_equal(hi, wm["last_j"])


def test_identical_sequences_come_back():
    y = np.array(MR.make_stack("soft", 3, (9,)))
    for S, tile in ((1, (4, 4)), (3, (4, 4)), (3, TILE)):
        got = MR.barycenter([y] * S, 0, 10, 1e-6, tile)
        assert got["inertia"] == [0.0, 0.0] and got["n_iter"] == 1 and got["reason"] == "converged"
        assert np.array_equal(got["template"].view(np.int32), y.view(np.int32)) and np.all(got["count"] == S)


def test_copies_with_repeated_rows_keep_the_base():
    base, copies, picks, _ = MR.planted(3, 20, 3, seed=2, noise=0.0)
    got = MR.barycenter(copies, base, 10, 1e-6, (8, 8))
    assert got["inertia"] == [0.0, 0.0] and np.array_equal(got["template"].view(np.int32), base.view(np.int32))
    for p, pick in zip(got["paths"], picks):
        assert np.array_equal(p[:, 0], pick[p[:, 1]])       # every copy row is aligned with the base row it repeats


def test_update_does_not_raise_the_objective_for_fixed_paths():
    """For fixed paths the objective splits by template entry: f(t) = cnt (t - mu)^2 + const with mu the exact mean of the
    aligned values, so any t' has f(t') - f(mu) = cnt (t' - mu)^2 and f(mu) <= f(t).  T' is mu computed in f64 (cnt additions and
    one division: |mu64 - mu| <= (cnt + 1) 2^-53 max|y| to first order) rounded once to f32 (|T' - mu64| <= 2^-24 |mu64|).
    Hence f(T') <= f(T) + sum_il cnt_i (2^-24 |T'_il| (1 + 2^-23) + (cnt_i + 1) 2^-52 max|y|)^2, plus the error of the
    comparison itself: every product under math.fsum is rounded once, at most 2^-52 of each objective."""
    for _, T, lengths, L in MR.update_cases(TI):
        tmpl, seqs, res, ranges, (new, count) = MR.update_case(T, lengths, L, TI, TJ)
        paths = [r["path"] for r in res]
        before, after = MR.objective(tmpl, seqs, paths), MR.objective(new, seqs, paths)
        ymax = max(float(np.abs(y).max()) for y in seqs)
        c = count.astype(np.float64)[:, None]
        slack = float((c * (2.0 ** -24 * np.abs(new.astype(np.float64)) * (1 + 2.0 ** -23) + (c + 1) * 2.0 ** -52 * ymax) ** 2).sum())
        slack += 2.0 ** -52 * (before + after)
        print(f"T={T} lengths={lengths} L={L}: objective {before!r} -> {after!r}, slack {slack!r}")
        assert after <= before + slack
        assert slack < 1e-9 * before                        # the slack is rounding, not room


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_planted_copies(seed):
    """noisy warped copies of a clean chain: the inertia never rises before the stop, and the barycenter lies nearer to the clean
    chain than the most typical copy does (seeds 3, 4 and 5 of _dtw_many_ref.planted at S = 4, n = 40, L = 3, noise 0.3)"""
    base, copies, _, _ = MR.planted(4, 40, 3, seed=seed, noise=0.3)
    tile = (16, 16)
    got = MR.barycenter(copies, "medoid", 8, 1e-6, tile)
    h = got["inertia"]
    upto = h[:-1] if got["reason"] == "increased" else h
    assert all(b <= a for a, b in zip(upto, upto[1:])) and len(h) >= 3
    assert got["reason"] != "increased" or h[-1] > min(h[:-1])
    k = MR.medoid(MR.distance_matrix(copies, "sqeuclidean", tile)["cost"])["index"]
    to_base = lambda t: R.dtw(t, base, "sqeuclidean", tile=tile)["cost"]     # noqa: E731
    print(f"seed {seed}: inertia {h}, {got['reason']}; to the clean chain: barycenter {to_base(got['template'])}, "
          f"medoid {to_base(copies[k])}")
    assert to_base(got["template"]) < to_base(copies[k])


def test_cost_is_symmetric_bit_for_bit():
    lengths = MR.stack_lengths(TI)
    for kind, L in (("soft", 50), ("repeat", 50), ("code", 50)):
        seqs = MR.split(MR.make_stack(kind, L, lengths), lengths)
        for metric in R.metrics_of(kind):
            for a, b in MR.all_pairs(len(lengths)):
                ab, ba = R.dtw(seqs[a], seqs[b], metric, tile=TILE), R.dtw(seqs[b], seqs[a], metric, tile=TILE)
                assert _bits([ab["cost"]]) == _bits([ba["cost"]]), (kind, metric, a, b)


# ---- the defects have teeth on the GPU test's cases ---------------------------------------------------------------------------------------

def _pair_differs(a, b):
    return (a["path"] is None or not np.array_equal(a["packed"], b["packed"]) or not np.array_equal(a["path"], b["path"])
            or not np.array_equal(_bits(a["last_row"]), _bits(b["last_row"])))


@pytest.mark.parametrize("defect", MR.DEFECTS)
def test_every_defect_shows_on_the_gpu_cases(defect):
    lengths = MR.stack_lengths(TI)
    if defect in ("pair_row_offset", "shared_frontier", "launches_of_first_pair"):
        X = MR.make_stack("soft", 50, lengths)
        shown = 0
        for second in (False, True):
            pairs = MR.SECOND_BATCH if second else MR.all_pairs(len(lengths))
            ref = MR.stack_reference("soft", 50, "sqeuclidean", TI, TJ, second)
            bad = MR.align_pairs(X, lengths, X, lengths, pairs, "sqeuclidean", TILE, defect)
            shown += any(_pair_differs(g, r) for g, r in zip(bad, ref))
        assert shown >= 1
    elif defect in ("range_off_by_one", "update_sum_f32", "update_divides_by_S"):
        shown = 0
        for _, T, lens, L in MR.update_cases(TI):
            tmpl, seqs, res, ranges, (new, count) = MR.update_case(T, lens, L, TI, TJ)
            bad_ranges = [MR.path_ranges(r["path"], T, defect) for r in res]
            bad, _ = MR.update(seqs, bad_ranges, T, defect)
            shown += not np.array_equal(bad.view(np.int32), new.view(np.int32))
        assert shown >= 2
    elif defect == "stale_paths_returned":
        c = MR.DBA_CASE
        _, copies, _, _ = MR.planted(c["S"], c["n"], c["L"], c["seed"])
        assert (0, 2) in MR.DBA_RUNS
        ref = MR.dba_reference(0, TI, TJ, 2)
        bad = MR.barycenter(copies, 0, 2, c["tol"], TILE, defect)
        assert ref["n_iter"] >= 1 and any(not np.array_equal(a, b) for a, b in zip(bad["paths"], ref["paths"]))
    elif defect == "medoid_tie_high":
        assert MR.medoid(MR.MEDOID_TIE)["index"] == 0 and MR.medoid(MR.MEDOID_TIE, defect)["index"] == 2
    else:
        v = MR.VOTE_CASE
        assert MR.vote(v["paths"], v["labels"], v["M"], v["K"]).tolist() == [0, 0]
        assert MR.vote(v["paths"], v["labels"], v["M"], v["K"], defect).tolist() == [1, 0]


# ---- the host functions -----------------------------------------------------------------------------------------------------------------

def test_medoid_and_votes_on_the_host():
    got, ref = sfv.dtw_medoid(MR.MEDOID_TIE), MR.medoid(MR.MEDOID_TIE)
    assert got["index"] == ref["index"] == 0 and np.array_equal(_bits(got["total"]), _bits(ref["total"]))
    assert got["total"].tolist() == [5.0, 6.0, 5.0, 8.0] and np.array_equal(_bits(got["mean_to_others"]), _bits(ref["total"] / 3))
    r = np.random.RandomState(0)
    c = r.rand(6, 6) * 1e3
    c = c + c.T
    np.fill_diagonal(c, 0.0)
    got, ref = sfv.dtw_medoid(c), MR.medoid(c)
    assert got["index"] == ref["index"] and np.array_equal(_bits(got["total"]), _bits(ref["total"]))
    assert sfv.dtw_medoid(np.zeros((1, 1)))["mean_to_others"].tolist() == [0.0]
    v = MR.VOTE_CASE
    carried = [sfv.transfer_labels(p, la, v["M"]) for p, la in zip(v["paths"], v["labels"])]
    assert sfv.vote_labels(carried).tolist() == MR.vote(v["paths"], v["labels"], v["M"], v["K"]).tolist() == [0, 0]
    # ties go to the smallest label, -1 abstains, and a row nobody votes on is -1
    votes = [[2, 1, -1, 3, -1], [1, 1, -1, 0, 4], [1, 2, -1, 3, -1], [2, 2, -1, 0, -1]]
    assert sfv.vote_labels(votes).tolist() == MR.vote_vectors(votes).tolist() == [1, 1, -1, 0, 4]
    assert sfv.vote_labels([np.array([3, -1])]).dtype == np.int64
    for call, match in ((lambda: sfv.vote_labels([]), "at least one"), (lambda: sfv.vote_labels([[0, 1], [0]]), "one length"),
                        (lambda: sfv.vote_labels([[0, -2]]), "non-negative"), (lambda: sfv.dtw_medoid(np.zeros((2, 3))), "S, S")):
        with pytest.raises(ValueError, match=match):
            call()
