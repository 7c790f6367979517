"""CPU: tests/_segment_ref.py (the f64 restatement the GPU tests compare csrc/segment.hip with) against its own long
double form on every layer case, against a brute-force enumeration of all segmentations on tiny inputs and against
planted boundaries; segments.boundary_agreement on hand-written lists; and the limits of rbvae_segment_ok, which needs
the library but no GPU.
"""
import ctypes
import math

import numpy as np
import pytest

import _segment_ref as R
import sfv_amd as sfv


@pytest.mark.parametrize("shape", R.PREFIX_SHAPES)
def test_prefix_within_bounds_of_long_double(shape):
    N, L = shape
    X, _ = R.case("soft", N, L, 2)
    P, Q = R.prefix(X)
    Pl, Ql = R.prefix(X, R.LD)
    assert np.all(P[0] == 0.0) and Q[0] == 0.0
    wp = R.within(P, Pl.astype(np.float64), R.p_bound(X) + R.U * np.abs(P), f"P {shape}")
    wq = R.within(Q, Ql.astype(np.float64), R.q_bound(X) + R.U * np.abs(Q), f"Q {shape}")
    print(f"prefix {shape}: worst |err|/bound P {wp:.3g}, Q {wq:.3g}")
    C, _ = R.case("code", N, L, 2)
    assert R.is_exact(C) and not R.is_exact(X)
    Pc, Qc = R.prefix(C)
    Pcl, Qcl = R.prefix(C, R.LD)
    assert np.array_equal(Pc, Pcl.astype(np.float64)) and np.array_equal(Qc, Qcl.astype(np.float64))      # exact integers


@pytest.mark.parametrize("which", ["D2", "random"])
@pytest.mark.parametrize("kind,N,L,S,m", R.LAYER_CASES)
def test_restatement_within_bounds_of_long_double(kind, N, L, S, m, which):
    _, _, _, prev, out, arg = R.layer_case(kind, N, L, S, m, which)
    ref = R.layer_case_ld(kind, N, L, S, m, which)
    assert np.isinf(prev).sum() > (0 if which == "D2" else 0.2 * N)
    worst, und = R.check_layer(kind, out, arg, ref, f"layer {(kind, N, L, S, m, which)}")
    rows = int((ref["n_cand"] > 0).sum())
    print(f"layer {(kind, N, L, S, m, which)}: worst |err|/bound {worst:.3g}, {und} of {rows} rows undecided")


def test_restatement_split_independent():
    """the minimum does not depend on how the ends are blocked"""
    kind, N, L, S, m = R.LAYER_CASES[4]
    _, P, Q, prev, out, arg = R.layer_case(kind, N, L, S, m, "random")
    rows = R.ROWS
    try:
        R.ROWS = 37
        out2, arg2 = R.layer(P, Q, prev, m)
    finally:
        R.ROWS = rows
    assert np.array_equal(out.view(np.int64), out2.view(np.int64)) and np.array_equal(arg, arg2)


@pytest.mark.parametrize("N,L,K,m", R.BRUTE_CASES)
def test_table_and_trace_against_brute_force(N, L, K, m):
    X = np.random.RandomState(N + L).rand(N, L).astype(np.float32)
    cost, arg, _, _ = R.table(X, K, m)
    cuts = R.trace(cost, arg)
    costs, best = R.brute(X, K, m)
    for k in range(1, K + 1):
        if best[k - 1] is None:
            assert np.isposinf(cost[k - 1, N]) and np.all(cuts[k - 1] == -1)
            continue
        assert abs(cost[k - 1, N] - costs[k - 1]) <= 1e-12, (k, cost[k - 1, N], costs[k - 1])
        assert tuple(cuts[k - 1, :k - 1]) == best[k - 1] and np.all(cuts[k - 1, k - 1:] == -1)
    assert best[K - 1] is not None
    assert np.all(np.diff(cost[:, N]) <= 1e-12)            # one more segment never costs more


@pytest.mark.parametrize("kind,N,L,S,m", R.PLANTED_CASES)
def test_planted_boundaries_recovered(kind, N, L, S, m):
    X, planted = R.case(kind, N, L, S)
    assert np.diff(np.concatenate([[0], planted, [N]])).min() >= m
    cost, arg, _, _ = R.table(X, S, m)
    cuts = R.trace(cost, arg)
    assert np.array_equal(cuts[S - 1, :S - 1], planted)


def test_boundary_agreement():
    f = sfv.boundary_agreement
    both = f([], [])
    assert (both["precision"], both["recall"], both["f1"], both["n_matched"]) == (1.0, 1.0, 1.0, 0)
    assert math.isnan(both["mean_abs_offset"])
    for a, b in (([], [5]), ([5], [])):
        one = f(a, b, 3)
        assert (one["precision"], one["recall"], one["f1"], one["n_matched"]) == (0.0, 0.0, 0.0, 0)
        assert math.isnan(one["mean_abs_offset"])
    same = f([10, 20, 30], [10, 20, 30])
    assert (same["precision"], same["recall"], same["f1"], same["n_matched"], same["mean_abs_offset"]) == (1.0, 1.0, 1.0, 3, 0.0)
    inside = f([12, 20, 29], [10, 20, 30], 2)               # shifts of 2, 0 and 1: inside the tolerance
    assert inside["n_matched"] == 3 and inside["f1"] == 1.0 and inside["mean_abs_offset"] == 1.0
    outside = f([13, 20, 29], [10, 20, 30], 2)              # the shift of 3 is outside
    assert outside["n_matched"] == 2 and outside["precision"] == 2 / 3 and outside["recall"] == 2 / 3
    assert abs(outside["f1"] - 2 / 3) < 1e-15 and outside["mean_abs_offset"] == 0.5
    assert f([13, 20, 29], [10, 20, 30])["n_matched"] == 1 and f([13], [10])["f1"] == 0.0
    rivals = f([9, 11], [10], 2)                            # two predictions for one truth: only the first is matched
    assert rivals["n_matched"] == 1 and rivals["precision"] == 0.5 and rivals["recall"] == 1.0
    assert abs(rivals["f1"] - 2 / 3) < 1e-15 and rivals["mean_abs_offset"] == 1.0
    rivals = f([10], [9, 11], 2)                            # and two truths for one prediction
    assert rivals["n_matched"] == 1 and rivals["precision"] == 1.0 and rivals["recall"] == 0.5
    assert f(np.array([4, 8]), np.array([8]), 0)["n_matched"] == 1          # the smaller advances first
    with pytest.raises(ValueError, match="sorted"):
        f([3, 2], [1])
    with pytest.raises(ValueError, match="tolerance"):
        f([1], [1], -1)


NEW = ("rbvae_segment_ok", "rbvae_segment_ws_bytes", "rbvae_segment_prefix", "rbvae_segment_layer", "rbvae_segment_trace")


def test_header_and_library():
    protos = sfv._lib.parse_header()
    raw = ctypes.CDLL(sfv._lib.LIB_PATH)
    for name in NEW:
        assert name in protos and hasattr(raw, name), name
    assert [len(protos[n][1]) for n in NEW] == [4, 2, 6, 10, 6]
    assert sfv._lib.query("rbvae_version") >= 102
    q = sfv._lib.query
    for ok in ((2, 1, 1, 1), (2, 1, 2, 1), (65536, 128, 256, 256), (12298, 50, 17, 1), (65536, 1, 1, 65536), (512, 3, 256, 2)):
        assert q("rbvae_segment_ok", *ok) == 1, ok
    for bad in ((1, 1, 1, 1), (8, 0, 2, 1), (8, 129, 2, 1), (300, 3, 257, 1), (65537, 3, 2, 1), (8, 3, 0, 1), (8, 3, 2, 0),
                (8, 3, 3, 3), (8, 3, 9, 1), (65536, 3, 256, 257), (8, 3, 2, -1)):
        assert q("rbvae_segment_ok", *bad) == 0, bad
    assert q("rbvae_segment_ws_bytes", 1, 1) == 0 and q("rbvae_segment_ws_bytes", 8, 129) == 0
    assert q("rbvae_segment_ws_bytes", 65537, 2) == 0
    assert q("rbvae_segment_ws_bytes", 64, 3) == 65 * 12 + 4               # one run of start tiles, rounded up to 8 bytes
    assert q("rbvae_segment_ws_bytes", 12298, 50) == (25 * 12299 * 12 + 7) // 8 * 8       # 193 end blocks in runs of 8 tiles
    assert q("rbvae_segment_ws_bytes", 65536, 128) == 32 * 65537 * 12      # never more than 32 runs
    for name in ("SegmentTable", "SegmentResult", "segment_prefix", "segment_layer", "segment_table", "segment",
                 "boundary_agreement", "latent_segments"):
        assert hasattr(sfv, name), name
