"""CPU: the LSTM cell-by-cell checker of tests/_lstm_cases.py is neither vacuous nor too tight, and its restated dispatch
reaches every kernel instance.

* an f32 emulation of the cell (f32 dot products, exp2 / reciprocal activations, the fused multiply-add of the cell state,
  the f32 BPTT with the recomputed tanh, an f32 weight gradient) passes every check in all three data regimes;
* a float64 result rounded to f32 passes;
* each of fourteen single defects, injected into otherwise exact data, fails the check that should see it;
* the case tables cover REACHABLE, and the first T at which each entry point changes kernel or refuses is reported."""
import pytest
import torch

import _lstm_cases as C

SHAPES = [(32, 4, 3, 6), (25, 2, 2, 5), (7, 3, 2, 4), (100, 2, 2, 3)]


def _data(L, layers, S, T, regime, seed=0):
    g = torch.Generator().manual_seed(100 * L + layers + seed)
    w = C.make_weights(L, layers, regime, g)
    x = torch.randn(S, T, L, generator=g)
    gt = torch.randn(S, T, L, generator=g)
    return w, x, gt


def _run_all(w, x, gt, L, layers, f32, defect=None, prev=None):
    """Forward, backward and weight gradient (each from the exact upstream data, so one defect is seen by one check)."""
    hs, hp, acts, cs = C.forward_pass(w, x, L, layers, f32=f32, defect=defect)
    hs0, hp0, acts0, cs0 = C.forward_pass(w, x, L, layers)            # exact saved state: the backward's inputs
    dG, dx = C.backward_pass(w, acts0, cs0, gt, L, layers, f32=f32, defect=defect)
    dG0, _ = C.backward_pass(w, acts0, cs0, gt, L, layers)
    gb = C.wgrad_pass(dG0, hs0, hp0, L, layers, f32=f32, prev=prev, defect=defect)
    return dict(hs=hs, hp=hp, acts=acts, cs=cs, acts0=acts0, cs0=cs0, dG=dG, dx=dx, dG0=dG0, hs0=hs0, hp0=hp0, gb=gb)


def _check_all(w, gt, r, L, layers, prev=None):
    out = dict(C.check_forward(w, r["hs"], r["hp"], r["acts"], r["cs"], L, layers))
    out.update(C.check_backward(w, r["acts0"], r["cs0"], gt.double(), 0.0, r["dG"], r["dx"], L, layers))
    out["wgrad"] = C.check_wgrad(r["dG0"], r["hs0"], r["hp0"], r["gb"], L, layers, prev=prev)
    return out


@pytest.mark.parametrize("regime", C.REGIMES)
@pytest.mark.parametrize("f32", [True, False], ids=["f32-emulation", "f64-rounded"])
def test_emulation_and_rounded_reference_pass(regime, f32):
    worst = {}
    for L, layers, S, T in SHAPES:
        w, x, gt = _data(L, layers, S, T, regime)
        prev = torch.randn(layers * C.layer_floats(L), generator=torch.Generator().manual_seed(3)) if L == 25 else None
        r = _run_all(w, x, gt, L, layers, f32, prev=prev)
        for t in (r["hs"], r["acts"], r["cs"], r["dG"], r["dx"], r["gb"]):
            assert torch.isfinite(t).all()
        for k, v in _check_all(w, gt, r, L, layers, prev=prev).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"BOUNDS lstm cpu {'f32 emulation' if f32 else 'f64 rounded'} {regime}: "
          + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0
    if regime == "saturated" and f32:
        assert worst["gates"] > 0.0


def test_saturated_regime_really_saturates():
    """+-100 biases: exp2's argument passes +-128, so the f32 emulation sees inf and 0 -- and stores exact 0 / 1 gates."""
    L, layers = 32, 2
    w, x, _ = _data(L, layers, 2, 3, "saturated")
    acts = C.forward_pass(w, x, L, layers, f32=True)[2]
    assert bool((acts == 0).any()) and bool((acts == 1).any()) and torch.isfinite(acts).all()
    w2, x2, _ = _data(L, layers, 2, 3, "wide")
    a2 = C.forward_pass(w2, x2, L, layers)[2][..., :2 * L]
    assert float(a2.min()) < 1e-3 and float(a2.max()) > 1 - 1e-3          # gates near 0 and 1


FORWARD_DEFECTS = [("gate_order", "gates of layer 0"), ("drop_bhh", "gates of layer"), ("skip_last_k", "gates of layer 0"),
                   ("h_from_prev_seq", "hprev"), ("c_not_reset", "cell state of layer 1"), ("sigmoid_g", "gates of layer 0")]
BACKWARD_DEFECTS = [("cprev_t0", "dG of layer"), ("dc_no_f", "dG of layer"), ("dx_swap", ": dx")]
WGRAD_DEFECTS = [("bias_nonzero_rows", "lstm wgrad"), ("edge_tile", "lstm wgrad"), ("accumulate_overwrites", "lstm wgrad")]


@pytest.mark.parametrize("defect,seen_by", FORWARD_DEFECTS + BACKWARD_DEFECTS + WGRAD_DEFECTS)
@pytest.mark.parametrize("L,layers,S,T", [(25, 2, 3, 5), (32, 4, 2, 4)])
def test_single_defects_fail_their_check(defect, seen_by, L, layers, S, T):
    w, x, gt = _data(L, layers, S, T, "small", seed=1)
    prev = torch.randn(layers * C.layer_floats(L), generator=torch.Generator().manual_seed(4))
    clean = _run_all(w, x, gt, L, layers, False, prev=prev)
    _check_all(w, gt, clean, L, layers, prev=prev)                     # otherwise exact data passes
    r = _run_all(w, x, gt, L, layers, False, defect=defect, prev=prev)
    with pytest.raises(AssertionError, match=seen_by):
        _check_all(w, gt, r, L, layers, prev=prev)
    # ... and only that family of checks: the other two still pass on the defective run
    fam = "fwd" if (defect, seen_by) in FORWARD_DEFECTS else "bwd" if (defect, seen_by) in BACKWARD_DEFECTS else "wgrad"
    if fam != "fwd":
        C.check_forward(w, r["hs"], r["hp"], r["acts"], r["cs"], L, layers)
    if fam != "bwd":
        C.check_backward(w, r["acts0"], r["cs0"], gt.double(), 0.0, r["dG"], r["dx"], L, layers)
    if fam != "wgrad":
        C.check_wgrad(r["dG0"], r["hs0"], r["hp0"], r["gb"], L, layers, prev=prev)


def test_cast_defects_fail_the_cast_check():
    g = torch.Generator().manual_seed(8)
    src = torch.randn(6, 25, generator=g)
    for dt in (torch.bfloat16, torch.float32):
        cast = torch.zeros(6, 64, dtype=dt)
        cast[:, :25] = src.to(dt)
        C.check_cast(cast, src, 25)
        bad = cast.clone()
        bad[3, 40] = 1e-30                                                  # a non-zero padding column
        with pytest.raises(AssertionError, match="cast"):
            C.check_cast(bad, src, 25)
    trunc = torch.zeros(6, 64, dtype=torch.bfloat16)
    trunc[:, :25] = (src.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)      # rounded by truncation
    one_row = torch.zeros(6, 64, dtype=torch.bfloat16)
    one_row[:, :25] = src.to(torch.bfloat16)
    one_row[2] = trunc[2]
    assert not torch.equal(one_row[2, :25], src[2].to(torch.bfloat16)), "the row has no element where truncation differs"
    with pytest.raises(AssertionError, match="cast"):
        C.check_cast(one_row, src, 25)


def test_slab_sums_and_colsum_and_binarise_checks():
    g = torch.Generator().manual_seed(9)
    parts = torch.randn(5, 40, generator=g)
    assert torch.equal(C.slab_sum_fwd(parts), C.slab_sum_bwd(parts))         # the same left-to-right f32 sum
    dx = torch.randn(3, 7, 25, generator=g)
    C.check_colsum(dx.sum(1), dx)
    bad = dx.sum(1)
    bad[1, 3] += dx[1, 6, 3]                                                  # one row counted twice
    with pytest.raises(AssertionError, match="dx_colsum"):
        C.check_colsum(bad, dx)
    # binarise forward: f32 arithmetic passes, a wrong temperature or a soft code where a hard one belongs fails
    h, Un = torch.randn(12, 25, generator=g), torch.rand(12, 25, generator=g)
    n = 0.3 * (torch.log(Un + 1e-8) - torch.log(1 - Un + 1e-8))
    y = torch.sigmoid((h + n) / 0.6)
    C.check_binarize(h, Un, y, (y > 0.5).float(), 0.6, 0.3, 1e-8, 1)
    C.check_binarize(h, Un, y, y, 0.6, 0.3, 1e-8, 0)
    with pytest.raises(AssertionError, match="y_soft"):
        C.check_binarize(h, Un, torch.sigmoid((h + n) / 0.6001), y, 0.6, 0.3, 1e-8, 0)
    with pytest.raises(AssertionError, match="codes"):
        C.check_binarize(h, Un, y, y, 0.6, 0.3, 1e-8, 1)
    z = (y > 0.5).float().reshape(3, 4, 25)
    kl = C.kl_elem64(z.double().reshape(3, -1), float(torch.tensor(0.1)), 1e-8, 1).sum(1).float()
    C.check_kl_parts(kl, z, 3, 0.1, 1e-8, 1)
    with pytest.raises(AssertionError, match="kl_parts"):
        C.check_kl_parts(kl * (1 + 1e-5), z, 3, 0.1, 1e-8, 1)
    # binarise backward: the f32 formula passes its bound; dropping the KL term does not
    gz, ghs = torch.randn(12, 25, generator=g), torch.randn(12, 25, generator=g)
    kg = torch.autograd.functional.jacobian(lambda v: C.kl_elem64(v, float(torch.tensor(0.1)), 1e-8, 0).sum(), y.double())
    ref, E = C.gtop_bin(gz.double(), 0.0, y, y, ghs, 0.7, 1.0, 12, 0.1, 1e-8, 0)
    want = ghs.double() + (gz.double() + (1.0 / 12) * kg) * y.double() * (1 - y.double()) / float(torch.tensor(0.7))
    assert float(((ref - want).abs() / E).max()) < 1.0
    assert float(((ref.float().double() - ref).abs() / E).max()) <= 1.0
    no_kl = ghs + gz * y * (1 - y) / 0.7
    assert float(((no_kl.double() - ref).abs() / E).max()) > 1.0


def test_dispatch_reaches_every_instance_and_reports_the_boundaries():
    got = C.covered_instances()
    missing = [k for k in C.REACHABLE if k not in got]
    assert not missing, missing
    assert not [k for k in got if isinstance(k, tuple)], "a case of the positive tables is refused by the dispatch"
    assert not [k for k in got if k not in C.REACHABLE], "the dispatch names a kernel outside REACHABLE"
    for c in C.FWD_REFUSALS:
        assert C.fwd_instance(c)[0] == "refused", c
    for c in C.BWD_REFUSALS:
        assert C.bwd_instance(c)[0] == "refused", c
    for which, c in C.PAIR_REFUSALS:
        f = C.pair_fwd_dispatch if which == "fwd" else C.pair_bwd_dispatch
        assert f(c["T"], c["L"], c["layers"])[0] == "refused", c
    for L, layers in ((32, 4), (25, 2)):
        for entry, (T, what) in C.first_changes(L, layers).items():
            print(f"DISPATCH lstm L={L} layers={layers} {entry}: first change at T={T} -> {what}")
    fc = C.first_changes(32, 4)
    # the wavefront kernels' ranges as include/rbvae_hip.h states them
    assert fc["rbvae_lstm_fwd"][0] == 100 and fc["rbvae_lstm_bwd"][0] == 23
    assert fc["rbvae_lstm_bwd_bin"][1][0] == "refused" and fc["rbvae_lstm_fwd_ex"][1][0] == "refused"
    # the big kernels refuse long sequences (the layer-sequential kernels serve L <= 32 only)
    for L in (50, 100, 128):
        assert C.first_change(lambda T: C.bwd_dispatch(T, L, 1)) == (21, ("refused", "T too long"))
    assert [C.first_change(lambda T: C.fwd_dispatch(T, L, 1))[0] for L in (50, 100, 128)] == [32, 23, 21]
    # shapes the issue asks for
    Ls = {c["L"] for c in C.FWD_CASES} | {c["L"] for c in C.BWD_CASES}
    assert {7, 24, 25, 28, 31, 32, 33, 40, 50, 64, 75, 88, 100, 125, 128} <= Ls and Ls & {1, 2} and Ls & {101, 112}
    assert {c["nparts"] for c in C.FWD_CASES + C.BWD_CASES} >= {1, 2, 3, 4, 5}
    assert {c["S"] * c["T"] for c in C.WGRAD_CASES} >= {1, 3, 4, 5, 63, 64, 65, 257}
    for tab in (C.FWD_CASES, C.BWD_CASES, C.PAIR_FWD_CASES, C.PAIR_BWD_CASES, C.WGRAD_CASES):
        assert {c["regime"] for c in tab} == set(C.REGIMES)


def test_restated_ranges_equal_the_library_queries():
    """The four range queries are plain host functions: the restated arithmetic agrees with them on a grid that crosses
    every boundary (they need no GPU)."""
    import sfv_amd
    q = sfv_amd._lib.query
    for L in (1, 7, 16, 17, 25, 28, 31, 32, 33, 64):
        for layers in (1, 2, 4, 5, 8, 9):
            for T in list(range(1, 130)) + [215, 216, 217, 253, 254, 1000]:
                assert bool(q("rbvae_lstm_fwd_wave_ok", T, L, layers)) == C.fwd_wave_ok(T, L, layers), (T, L, layers)
                assert bool(q("rbvae_lstm_bwd_wave_ok", T, L, layers)) == C.bwd_wave_ok(T, L, layers), (T, L, layers)
                assert bool(q("rbvae_lstm_pair_fwd_ok", T, L, layers)) == C.pair_fwd_ok(T, L, layers), (T, L, layers)
                assert bool(q("rbvae_lstm_pair_bwd_ok", T, L, layers)) == C.pair_bwd_ok(T, L, layers), (T, L, layers)
                # the two-stack launches never accept what the single-stack wavefront kernels refuse (the engine relies on it)
                assert not C.pair_fwd_ok(T, L, layers) or C.fwd_wave_ok(T, L, layers)
                assert not C.pair_bwd_ok(T, L, layers) or C.bwd_wave_ok(T, L, layers)
