"""CPU checks of tests/_ldm_cases.py: the restated gates and rbvae_groupnorm_ws_floats agree with the library over a grid
that includes refusals; the case tables reach every kernel form and every route the dispatchers can take; an f32 emulation
of each kernel's arithmetic passes its own bound on every case (the bounds are satisfiable) while float64 arithmetic of
the same algorithm stays below 1e-3 of it; and each named defect is rejected on a named case (the bounds are not slack)."""
import pytest
import torch

import _ldm_cases as L

F32, F64 = torch.float32, torch.float64
ids = lambda cases: [c["id"] for c in cases]


def test_restated_gates_match_the_library_over_a_grid_with_refusals():
    import sfv_amd
    lib = sfv_amd._lib
    seen = set()
    for dtype in (0, 1, 2):
        for hw in (-32, 0, 1, 16, 31, 32, 48, 64, 96, 100, 128, 160, 1024, 4096):
            for C in (0, 32, 64, 96, 128, 192, 256, 512, 1024):
                want = L.attn_ok(dtype, hw, C)
                assert int(lib.query("rbvae_attention_ok", dtype, hw, C)) == want, (dtype, hw, C)
                seen.add(want)
    assert seen == {0, 1}
    tiled = set()
    for dtype in ("f32", "bf16"):
        for C, groups in ((4, 1), (8, 2), (32, 4), (36, 4), (64, 32), (64, 64), (96, 32), (128, 32), (128, 128), (256, 32),
                          (256, 64), (384, 32), (512, 32), (1024, 32), (2048, 32), (4096, 32), (100, 32)):
            for N, HW in ((1, 1), (3, 31), (2, 32), (1, 33), (3, 515), (2, 4096 + 5)):
                want = L.gn_ws_floats(dtype, N, HW, C, groups)
                assert int(lib.query("rbvae_groupnorm_ws_floats", L.DT[dtype], N, HW, C, groups)) == want, (dtype, N, HW, C, groups)
                tiled.add(want > 2 * N * groups)
    assert tiled == {False, True}
    assert (L.gn_rows_per_block("bf16", 512), L.gn_rows_per_block("f32", 256), L.gn_rows_per_block("f32", 1024)) == (32, 32, 8)
    assert L.gn_vec_index_ok("bf16", (1 << 32) - (1 << 22), 8) and not L.gn_vec_index_ok("bf16", (1 << 32) - (1 << 22) + 1, 8)


def test_case_tables_reach_every_form_and_route():
    assert {L.attn_form(c["C"], c["hw"]) for c in L.AT_CASES} == L.AT_REACHABLE
    shapes = {(c["C"], c["hw"]) for c in L.AT_CASES}
    assert shapes == {(C, hw) for C in (64, 128, 256) for hw in (32, 64, 96, 160)} | {(512, hw) for hw in (32, 96, 128, 160, 192, 1024)}
    for form in L.AT_REACHABLE:                     # every data kind on every kernel form, both layouts, both ldo
        mine = [c for c in L.AT_CASES if L.attn_form(c["C"], c["hw"]) == form]
        assert {c["kind"] for c in mine} == set(L.AT_KINDS), form
        assert {c["layout"] for c in mine} == {"fused", "split"} and {c["ldo"] - c["C"] for c in mine} == {0, 8}
        assert {c["N"] for c in mine} == {1, 2, 3}
    assert all(c["N"] >= 2 for c in L.AT_CASES if c["kind"] == "uniform")
    for hw in (32, 96, 160, 1024):
        p = L.peaked_perm(hw).tolist()
        assert {0, 31, 32 % hw, 63 % hw, hw - 32, hw - 1} <= set(p) and p[hw - 1] == 31

    routes = {L.gn_route(c)[:2] for c in L.GN_CASES}
    assert routes == L.GN_ROUTES
    assert {L.gn_route(c)[2] for c in L.GN_CASES if c["entry"] in ("swish_ws", "swish")} - {None} == L.GN_CAUSES
    for dt in ("f32", "bf16"):
        t = [c for c in L.GN_CASES if c["dtype"] == dt and L.gn_route(c)[0] == "gn_partial_k+gn_finish_k" and c["entry"] == "swish_ws"]
        assert {L.gn_route(c)[1] for c in t} == {"gn_apply_vec_k:cg4", "gn_apply_vec_k:cg_odd"}
        assert any(c["C"] == 64 and c["groups"] == 32 for c in t)
        rb = 32
        hws = {c["HW"] for c in t if L.gn_rows_per_block(dt, c["C"]) == rb}
        assert {1, rb - 1, rb, rb + 1, 3 * rb + 5} <= hws
        assert {c["N"] for c in t} == {1, 3} and {c["swish"] for c in t} == {0, 1}
        assert any(c["ldx"] > c["C"] and c["ldy"] > c["C"] for c in t)
    assert {c["groups"] for c in L.GN_CASES} >= {1, 4, 32, 64}
    assert {c["kind"] for c in L.GN_CASES} == {"offset", "far", "ramp", "const", "outlier"}
    assert any(L.cdiv(c["HW"], L.gn_rows_per_block(c["dtype"], c["C"])) > 64 for c in L.GN_CASES if L.gn_route(c)[2] is None)
    second = {L.gn_route(c)[1] for c in L.GN_CASES if c["entry"] == "apply" and
              (c["N"] * c["HW"] * c["C"] > 8192 * 256 if L.gn_route(c)[1] == "gn_apply_k"
               else c["N"] * c["HW"] * c["C"] // L.GN_V[c["dtype"]] > 16384 * 256)}
    assert second == {"gn_apply_k", "gn_apply_vec_k:cg4"}
    assert {c["n"] for c in L.SM_CASES} == {1, 63, 64, 65, 200} and any(c["rows"] % 4 for c in L.SM_CASES)
    assert {(c["dtype"], c["inplace"]) for c in L.SM_CASES} == {(d, i) for d in ("f32", "bf16") for i in (False, True)}
    assert {(c["R"], c["C"]) for c in L.TR_CASES} == {(1, 1), (1, 40), (33, 31), (64, 96), (100, 513)}
    assert any(c["N"] * c["Z"] * c["HW"] > 8192 * 256 for c in L.PS_CASES)
    assert {(c["dtype"], c["eps"], c["ld"] > 2 * c["Z"]) for c in L.PS_CASES} == {(d, e, p) for d in ("f32", "bf16")
                                                                                  for e in (False, True) for p in (False, True)}


@pytest.mark.parametrize("c", L.AT_CASES, ids=ids(L.AT_CASES))
def test_attention_emulation_passes(c):
    d, _, _ = L.at_case(c["id"])
    assert L.at_check(c, L.at_forward(c, d, F32)) <= 1.0
    assert L.at_check(c, L.at_forward(c, d, F64)) < 1e-3


AT_DEFECTS = [("skip_last_tile", "c512_hw128_n2_uniform_fused_ldo0"), ("skip_last_tile", "c64_hw96_n1_peaked_fused_ldo0"),
              ("skip_last_tile", "c512_hw160_n3_rising_split_ldo8"),
              ("key31_zero", "c512_hw32_n2_uniform_split_ldo0"), ("key31_zero", "c128_hw96_n2_peaked_split_ldo0"),
              ("key31_zero", "c64_hw64_n1_random_split_ldo0"),
              ("v_rot", "c256_hw32_n1_peaked_split_ldo0"), ("v_rot", "c512_hw128_n1_huge_split_ldo0"),
              ("no_log2e", "c64_hw64_n1_random_split_ldo0"), ("no_log2e", "c512_hw96_n3_huge_fused_ldo8"),
              ("alpha1_second", "c64_hw64_n2_rising_fused_ldo8"), ("alpha1_second", "c512_hw160_n2_peaked_fused_ldo8"),
              ("alpha1_second", "c512_hw128_n2_random_fused_ldo0"),
              ("image0_keys", "c64_hw32_n2_uniform_fused_ldo8"), ("image0_keys", "c512_hw128_n2_random_fused_ldo0"),
              ("image0_keys", "c128_hw96_n2_peaked_split_ldo0")]


@pytest.mark.parametrize("defect,case", AT_DEFECTS, ids=[f"{a}-{b}" for a, b in AT_DEFECTS])
def test_attention_defects_fail(defect, case):
    c = L.by_id(L.AT_CASES, case)
    d, _, _ = L.at_case(case)
    with pytest.raises(AssertionError, match="worst"):
        L.at_check(c, L.at_forward(c, d, F64, defect))
    assert {a for a, _ in AT_DEFECTS} == set(L.AT_DEFECTS)


@pytest.mark.parametrize("c", L.GN_CASES, ids=ids(L.GN_CASES))
def test_groupnorm_emulation_passes(c):
    d, _ = L.gn_case(c["id"])
    r32, r64 = L.gn_check(c, L.gn_forward(c, d, F32)), L.gn_check(c, L.gn_forward(c, d, F64))
    assert max(r32.values()) <= 1.0 and max(r64.values()) < 1e-3
    if c["kind"] == "const" and "rstd" in r32:
        assert float(L.gn_case(c["id"])[1]["rstd"][0].max()) == pytest.approx(1000.0)


GN_DEFECTS = [("no_merge_term", "t_f32_c256_hw101_ramp"), ("no_merge_term", "t_bf16_c512_hw101_ramp"),
              ("no_merge_term", "t_bf16_c256_g64_hw70_outlier"), ("no_merge_term", "s_bf16_c128_hw300_offset_ld"),
              ("short_block_full", "t_f32_c256_hw33_outlier_ld"), ("short_block_full", "t_bf16_c512_hw101_ramp"),
              ("short_block_full", "s_f32_c256_hw101_ramp"),
              ("one_pass", "t_f32_c256_hw101_far"), ("one_pass", "f_f32_c384_hw20_far"), ("one_pass", "s_f32_c36_hw50_far")]


@pytest.mark.parametrize("defect,case", GN_DEFECTS, ids=[f"{a}-{b}" for a, b in GN_DEFECTS])
def test_groupnorm_defects_fail(defect, case):
    c = L.by_id(L.GN_CASES, case)
    d, _ = L.gn_case(case)
    with pytest.raises(AssertionError, match="worst"):
        L.gn_check(c, L.gn_forward(c, d, F32 if defect == "one_pass" else F64, defect))
    assert {a for a, _ in GN_DEFECTS} == set(L.GN_DEFECTS)


def test_groupnorm_apply_uses_the_given_statistics_and_the_neighbouring_group_fails():
    c = L.by_id(L.GN_CASES, "a_f32_c256_hw33")
    d, _ = L.gn_case(c["id"])
    bad = dict(d, mean=d["mean"].roll(1), rstd=d["rstd"].roll(1))
    with pytest.raises(AssertionError, match="worst"):
        L.gn_check(c, L.gn_forward(c, bad, F64))


@pytest.mark.parametrize("c", L.AF_CASES, ids=ids(L.AF_CASES))
def test_gn_affine_emulation_passes(c):
    d = L.af_data(c)
    ref = L.af_reference(c, d)
    for dt, lim in ((F32, 1.0), (F64, 1e-3)):
        got = L.af_forward(c, d, dt)
        for k, (r, b) in ref.items():
            assert L.check_bound(got[k], r, b, f"{c['id']} {k}") <= lim


@pytest.mark.parametrize("c", L.SM_CASES, ids=ids(L.SM_CASES))
def test_softmax_rows_emulation_passes(c):
    x = L.sm_data(c)
    ref, bnd = L.sm_reference(c, x)
    assert L.check_bound(L.sm_forward(c, x, F32), ref, bnd, c["id"]) <= 1.0
    assert L.check_bound(L.sm_forward(c, x, F64), ref, bnd, c["id"]) < 1e-3
    if c["rows"] > 1 and c["n"] > 1:
        assert float(x[1].max() - x[1].min()) > 200 and float(ref[1].min()) < 1e-45
        with pytest.raises(AssertionError, match="worst"):           # the neighbouring row's maximum
            L.check_bound(torch.softmax(x.double(), 1).roll(1, 0), ref, bnd, c["id"])


@pytest.mark.parametrize("c", L.PS_CASES, ids=ids(L.PS_CASES))
def test_posterior_sample_emulation_passes(c):
    d = L.ps_data(c)
    ref, bnd = L.ps_reference(c, d)
    assert L.check_bound(L.ps_forward(c, d, F32), ref, bnd, c["id"]) <= 1.0
    assert L.check_bound(L.ps_forward(c, d, F64), ref, bnd, c["id"]) < 1e-3
    lv = d["mom"].float()[:, c["Z"]:]
    assert float(lv.max()) >= 20 and float(lv.min()) <= -30 if c["N"] * c["HW"] >= 4 else True
    if c["eps"] and c["N"] * c["HW"] >= 4:
        m = d["mom"].double().reshape(c["N"], c["HW"], 2 * c["Z"]).permute(0, 2, 1)
        unclamped = float(torch.tensor(d["scale"], dtype=F32)) * (m[:, :c["Z"]] + torch.exp(0.5 * m[:, c["Z"]:]) * d["eps"].double())
        with pytest.raises(AssertionError, match="worst"):
            L.check_bound(unclamped.reshape(-1), ref, bnd, c["id"])


def test_transpose_patterns_hold_the_special_values():
    for c in L.TR_CASES:
        bits = L.tr_bits(c)
        assert bits.shape == (c["R"], c["C"]) and c["ldi"] >= c["C"] and c["ldo"] >= c["R"]
        f = bits.view(L.TDT[c["dtype"]])
        if bits.numel() >= 6:
            assert bool(torch.isnan(f.reshape(-1)[2:5]).all()) and bool(torch.isinf(f.reshape(-1)[5]))
        assert float(f.reshape(-1)[0]) == 0.0 and bool(torch.signbit(f.reshape(-1)[0]))
