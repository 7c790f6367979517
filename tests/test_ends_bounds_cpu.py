"""CPU checks of tests/_ends_cases.py: the restated gates agree with the library over a grid that includes refusals; the
case tables reach every template instance the dispatchers can launch; an f32 emulation of each operation passes its own
bound on every case (the bounds are satisfiable) and exact float64 data passes; and each named defect is rejected on a
named case -- among them the two-kernel arithmetic (Y rounded to bf16 before the gather), which is what shows that the
deconv_last_fused bound is not slack."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _ends_cases as E

ids = lambda cases: [c["id"] for c in cases]
by_id = lambda cases, i: next(c for c in cases if c["id"] == i)


def test_restated_gates_match_the_library_over_a_grid_with_refusals():
    import sfv_amd
    L = sfv_amd._lib
    grid = E.gate_grid()
    assert len({g[0] for g in grid}) == 8
    for name, args, want in grid:
        assert int(L.query(name, *args)) == want, (name, args, want)
    refused = {name for name, _, want in grid if want == 0}
    assert {"rbvae_conv_first_fused_ok", "rbvae_deconv_last_dgrad_blocks", "rbvae_wgrad_first_blocks", "rbvae_conv_in_ok",
            "rbvae_deconv_last_fused_parts", "rbvae_col2im_has_dcol"} <= refused
    assert E.dl_lds(64) == 26624 and E.dl_lds(128) == 53248        # one slice buffer; two (Y, 23680 bytes, fits in either)


def test_case_tables_reach_every_instance_the_dispatch_can_launch():
    assert {E.cf_instance(c["Cin"], c["mode"], c["Nout"]) for c in E.CF_CASES} == E.CF_REACHABLE
    assert {E.wf_instance(c["Cin"], c["mode"], c["Nout"]) for c in E.WF_CASES} == E.WF_REACHABLE
    assert {E.dl_instance(c["C1"]) for c in E.DL_CASES} == E.DL_REACHABLE
    assert {E.ci_instance(c["Cin"], c["Nout"]) for c in E.CI_CASES} == E.CI_REACHABLE
    assert {E.im_kernel(c) for c in E.IM_CASES} == {("im2col_fast_k", d, k) for d in ("f32", "bf16") for k in (0, 3, 4)}
    assert {(c["dtype"], E.c2_geom(c)[4]) for c in E.C2_CASES} == {(d, k) for d in ("f32", "bf16") for k in ("pix", "general")}
    # every case is inside its gate
    for c in E.CF_CASES:
        assert E.cf_shape_ok("bf16", c["Cin"], c["IH"], c["IW"], c["Nout"], c["N"])
    for c in E.WF_CASES:
        assert E.wf_shape_ok("bf16", c["Cin"], c["IH"], c["IW"], c["Nout"], c["N"]) and 1 <= c["ks"] <= E.s2_blocks(c["N"], c["IH"], c["IW"])
    for c in E.DL_CASES:
        assert E.dl_parts("bf16", c["N"], c["IH"], c["IW"], c["C1"], c["Cout"]) > 0 and 9 * c["Cout"] <= c["NYP"] <= 48
    for c in E.CI_CASES:
        assert E.conv_in_ok("bf16", c["Cin"], c["H"], c["W"], c["Nout"], c["N"], c["cg"])
    # what the issue lists: the lone first / last chunk, NQ on both sides of 64, ldo > Nout, every drop / bias / relu form
    m0 = [c for c in E.CF_CASES if c["mode"] == 0]
    assert {8, 24, 64, 72, 200, 248, 256} <= {c["Nout"] for c in m0}
    assert {(1, 1), (1, 33), (15, 17), (32, 64), (33, 65), (88, 160), (256, 256)} <= {(c["IH"], c["IW"]) for c in m0}
    assert {c["drop"] for c in m0} == {None, "seed", "seed_dev"} and {c["relu"] for c in m0} == {0, 1}
    assert {c["bias"] for c in m0} == {0, 1} and any(c["ldo"] > c["Nout"] for c in m0) and any(c["fmap"] == "gap" for c in m0)
    assert {c["Nout"] for c in E.WF_CASES} == {64, 128, 192, 256, 320, 512}
    # K-splits: one slice, one block per slice, and trailing slices that are empty
    kinds = set()
    for c in E.WF_CASES:
        sl = E.k_slices(E.s2_blocks(c["N"], c["IH"], c["IW"]), c["ks"])
        assert sl[0][0] == 0 and max(b for _, b in sl) == E.s2_blocks(c["N"], c["IH"], c["IW"])
        kinds.add("one" if c["ks"] == 1 else "empty" if any(a == b for a, b in sl) else "per_block" if all(b - a == 1 for a, b in sl) else "split")
    assert kinds == {"one", "empty", "per_block", "split"}
    assert {c["C1"] for c in E.DL_CASES} == {64, 128, 192, 256, 320} and {c["Cout"] for c in E.DL_CASES} == {1, 2, 3, 4}
    assert {(1, 1), (8, 16), (9, 17), (5, 37), (11, 20), (44, 80)} <= {(c["IH"], c["IW"]) for c in E.DL_CASES}
    assert any(c["NYP"] > E.cdiv(9 * c["Cout"], 8) * 8 for c in E.DL_CASES) and any(c["target"] is None for c in E.DL_CASES)
    assert any(c["target"] is not None and not c["dpre"] for c in E.DL_CASES) and sum(c["sat"] for c in E.DL_CASES) >= 2
    assert {c["cg"] for c in E.CI_CASES} == {4, 8, 16} and {c["Nout"] for c in E.CI_CASES} == {32, 64, 128, 256}


def test_block_order_and_k_slices():
    blk = E.block_of_rows(2, 9, 33)                       # 2 x 3 blocks per image: tbi fastest, then tai, then the image
    at = lambda n, y, x: int(blk[(n * 9 + y) * 33 + x])
    assert (at(0, 0, 0), at(0, 0, 16), at(0, 0, 32), at(0, 8, 0), at(0, 8, 32), at(1, 0, 0)) == (0, 1, 2, 3, 5, 6)
    assert E.k_slices(10, 7) == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 10), (10, 10), (10, 10)]
    assert E.k_slices(9, 4) == [(0, 3), (3, 6), (6, 9), (9, 9)]
    offs, total, fm = E.frame_layout(4, 10, (1, 2))       # [Bi = 1][2][T = 2] padded frames: view 0 of the item, then view 1
    assert offs == [0, 15, 30, 45] and fm == (2, 2, 30, 60, 15) and total == 60
    assert E.frame_layout(8, 10, (2, 2))[0] == [0, 15, 60, 75, 30, 45, 90, 105]


def test_keyed_dropout_restatement():
    keep = E.keyed_keep_mask(999, 136, 11, 0.2)
    assert 0.17 < 1.0 - keep.mean() < 0.23
    assert not np.array_equal(keep, E.keyed_keep_mask(999, 136, 12, 0.2))
    assert not np.array_equal(keep, E.keyed_keep_mask(999, 136, 11, 0.2, row_stride=144))
    assert np.array_equal(keep[0], E.keyed_keep_mask(999, 136, 11, 0.2, row_stride=144)[0])       # row 0: the same indices
    assert not np.array_equal(keep, E.keyed_keep_mask(999, 136, 11, 0.2, seed_dev=5))
    assert E.keyed_keep_mask(50, 64, 3, 0.0).all()


def test_col2im_fold_is_the_transposed_convolution():
    g = torch.Generator().manual_seed(4)
    N, C1, Cout, IH, IW = 2, 6, 3, 5, 7
    a, V, b = torch.randn(N, C1, IH, IW, generator=g).double(), torch.randn(C1, Cout, 3, 3, generator=g).double(), torch.randn(Cout).double()
    Y = torch.einsum("nchw,cotk->nhwtok", a, V.reshape(C1, Cout, 9, 1)).reshape(N * IH * IW, 9 * Cout)
    pre = E.c2_gather(dict(N=N, IH=IH, IW=IW, Cout=Cout), Y, b, torch.float64)[0]
    ref = F.conv_transpose2d(a, V, b, stride=2, padding=1, output_padding=1)
    assert float((pre - ref).abs().max()) < 1e-12


def _both(build, forward, check, c):
    d = build(c)
    out = {}
    for dt in (torch.float32, torch.float64):
        out[dt] = check(c, d, forward(c, d, dt))
    return d, out


@pytest.mark.parametrize("c", E.CF_CASES, ids=ids(E.CF_CASES))
def test_conv_first_emulation_passes(c):
    d, res = _both(E.cf_build, E.cf_forward, E.cf_check, c)
    assert res[torch.float64]["out"] < 1e-3 and res[torch.float32]["out"] <= 1.0


@pytest.mark.parametrize("c", E.WF_CASES, ids=ids(E.WF_CASES))
def test_wgrad_first_emulation_passes(c):
    d = E.wf_build(c)
    assert E.wf_check(c, d, E.wf_forward(c, d, torch.float32)) <= 1.0
    assert E.wf_check(c, d, E.wf_forward(c, d, torch.float64)) < 1e-3


@pytest.mark.parametrize("c", E.DL_CASES, ids=ids(E.DL_CASES))
def test_deconv_last_emulation_passes(c):
    d, res = _both(E.dl_build, E.dl_forward, E.dl_check, c)
    assert res[torch.float64]["xr"] < 1e-3 and res[torch.float32]["xr"] <= 1.0
    if c["sat"]:
        assert float(d["pre"].abs().max()) > 25.0


@pytest.mark.parametrize("c", E.CI_CASES, ids=ids(E.CI_CASES))
def test_conv_in_emulation_passes(c):
    _both(E.ci_build, E.ci_forward, E.ci_check, c)


@pytest.mark.parametrize("c", E.C2_CASES, ids=ids(E.C2_CASES))
def test_col2im_emulation_passes(c):
    _both(E.c2_build, E.c2_forward, E.c2_check, c)


def test_im2col_reference_is_the_unfold_of_the_frames():
    for c in E.IM_CASES:
        d = E.im_build(c)
        x, k, s = d["x"], 3, c["stride"]
        n, oh, ow, kh, kw, ci = 0, d["OH"] - 1, d["OW"] - 1, 0, 1, c["C"] - 1
        ih, iw = oh * s - 1 + kh, ow * s - 1 + kw
        want = float(x[n, ci, ih, iw].to(E.TDT[c["dtype"]])) if 0 <= ih < c["H"] and 0 <= iw < c["W"] else 0.0
        assert float(d["want"][(n * d["OH"] + oh) * d["OW"] + ow, (kh * 3 + kw) * c["C"] + ci]) == want
        assert float(d["want"][:, 9 * c["C"]:].abs().max() if c["Kpad"] > 9 * c["C"] else 0.0) == 0.0


# ---- every named defect is rejected on a named case ------------------------------------------------------------------------

CF_DEFECTS = [("khkw", "m0_c3_15x17_n64_gap"), ("khkw", "m1_c4_32x64_n72_exact"), ("pad0", "m0_c4_32x64_n72_exact"),
              ("halo_col", "m0_c3_33x65_n200_onepast"), ("halo_row", "m1_c3_33x65_n200_onepast"),
              ("ragged_row", "m0_c3_33x65_n200_onepast"),
              ("ragged_row", "m1_c1_33x65_n72"), ("ci_major", "m0_c4_32x64_n72_exact"), ("ci_major", "m1_c2_88x160_n248"),
              ("bias_second_chunk", "m0_c4_32x64_n72_exact"), ("drop_ldo", "m0_c3_33x65_n200_onepast"),
              ("gate_ge0", "m1_c2_1x33_n24"), ("gate_nan", "m1_c1_1x1_n8"), ("colsum_swap", "m1_c4_88x160_n256_native")]


@pytest.mark.parametrize("defect,case", CF_DEFECTS, ids=[f"{a}-{b}" for a, b in CF_DEFECTS])
def test_conv_first_defects_fail(defect, case):
    c = by_id(E.CF_CASES, case)
    d = E.cf_build(c)
    with pytest.raises(AssertionError):
        E.cf_check(c, d, E.cf_forward(c, d, torch.float64, defect))


WF_DEFECTS = [("kslice_off_by_one", "m0_c2_33x65_n128_ks7_empty"), ("kslice_off_by_one", "m1_c3_88x160_n256_ks4"),
              ("ci_major", "m0_c4_15x17_n320_ks3"), ("ci_major", "m1_c2_15x17_n512_ks_nblk")]


@pytest.mark.parametrize("defect,case", WF_DEFECTS, ids=[f"{a}-{b}" for a, b in WF_DEFECTS])
def test_wgrad_first_defects_fail(defect, case):
    c = by_id(E.WF_CASES, case)
    d = E.wf_build(c)
    with pytest.raises(AssertionError):
        E.wf_check(c, d, E.wf_forward(c, d, torch.float64, defect))


DL_DEFECTS = [("tap_parity", "k3_9x17_co3_mapped"), ("y_bf16", "k4_44x80_co4_mapped"), ("y_bf16", "one_9x17_co2"),
              ("no_gscale", "k2_8x16_co2_nyp48_gap"), ("sse_ragged", "k3_9x17_co3_mapped"), ("target_plane", "k5_11x20_co4_nyp48")]


@pytest.mark.parametrize("defect,case", DL_DEFECTS, ids=[f"{a}-{b}" for a, b in DL_DEFECTS])
def test_deconv_last_defects_fail(defect, case):
    c = by_id(E.DL_CASES, case)
    d = E.dl_build(c)
    got = E.dl_forward(c, d, torch.float64, defect)
    if defect in ("no_gscale", "sse_ragged", "target_plane"):
        # losses are checked against the STORED xr and the true target: a wrong dpre / sse / target read shows there
        with pytest.raises(AssertionError):
            E.dl_check(c, d, got)
        assert E.dl_check(c, d, dict(xr=got["xr"]))["xr"] < 1e-3
    else:
        with pytest.raises(AssertionError, match="xr worst"):
            E.dl_check(c, d, got)


def test_the_two_kernel_arithmetic_is_rejected_by_the_fused_bound_by_a_wide_margin():
    """Sensitivity of the deconv_last_fused bound: Y rounded to bf16 lands far outside it (the bound is not slack)."""
    c = by_id(E.DL_CASES, "k4_44x80_co4_mapped")
    d = E.dl_build(c)
    xr = E.dl_forward(c, d, torch.float64, "y_bf16")["xr"]
    s = torch.sigmoid(d["pre"])
    r = (xr - s).abs() / E.sigmoid_bound(d["pre"], d["S"], E.B.c_acc(4 * c["C1"]), lib=False)
    assert float(r.max()) > 20.0 and float((r > 1).double().mean()) > 0.5


C2_DEFECTS = [("tap_parity", "f32_co4_5x37_mapped"), ("no_gscale", "bf16_co3_11x20_mapped"), ("no_gscale", "f32_co5_general")]


@pytest.mark.parametrize("defect,case", C2_DEFECTS, ids=[f"{a}-{b}" for a, b in C2_DEFECTS])
def test_col2im_defects_fail(defect, case):
    c = by_id(E.C2_CASES, case)
    d = E.c2_build(c)
    with pytest.raises(AssertionError):
        E.c2_check(c, d, E.c2_forward(c, d, torch.float64, defect))


def test_conv_in_defect_fails():
    c = by_id(E.CI_CASES, "c3_n128_cg8_64x64")
    d = E.ci_build(c)
    with pytest.raises(AssertionError):
        E.ci_check(c, d, E.ci_forward(c, d, torch.float64, "khkw"))
    good = E.ci_forward(c, d, torch.float32)
    bad = dict(out=good["out"], stats=good["stats"].roll(1, 0))        # statistics of the neighbouring (tile, group)
    with pytest.raises(AssertionError):
        E.ci_check(c, d, bad)
