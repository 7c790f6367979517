"""The checker and the case tables of tests/_wgrad_cases.py without a GPU: the references of both roles are torch's
autograd, every table case's own reference (and the block-by-block emulation) passes its own check, each planted defect
of a stride-2 weight-gradient kernel fails one, the restated geometry equals the library's host queries, and the tables
reach every loop arm of wgrad_halo_k and wgrad_row_k<8> / <4> that the GPU test relies on."""
import pytest
import torch
import torch.nn.functional as F

import _wgrad_cases as W

CASE_IDS = [c["id"] for _, c in W.ALL_CASES]


def of(kind, data):
    return [c for c in W.TABLES[kind] if c["data"] == data]


# ---- the references ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("role", ["conv", "deconv"])
@pytest.mark.parametrize("data", ["int", "randn"])
def test_reference_of_both_roles_is_autograd(role, data):
    c = dict(id=f"cpu_{role}_{data}", N=3, OH=3, OW=5, Ca=8, Cb=16, ks=1, role=role, data=data)
    s, g = W.operands(c)
    ref, scale = W.reference(c, s, g)
    w = torch.zeros(8, 16, 3, 3, dtype=torch.float64, requires_grad=True)
    if role == "conv":                   # W [co = Ca][ci = Cb]: g is the input, s the output gradient
        F.conv2d(g.double(), w, None, stride=2, padding=1).backward(s.double())
    else:                                # W [ci = Ca][co = Cb]: s is the input, g the output gradient
        F.conv_transpose2d(s.double(), w, None, 2, 1, 1).backward(g.double())
    want = W.tap_layout(w.grad)
    torch.testing.assert_close(ref, want, rtol=1e-13, atol=1e-13)
    if data == "int":
        assert torch.equal(ref, want)
    assert bool((scale >= ref.abs()).all())


@pytest.mark.parametrize("kind,c", W.ALL_CASES, ids=CASE_IDS)
def test_every_table_case_reference_and_emulation_pass(kind, c):
    """int: the reference equals itself and the emulation's sum exactly, every emulated slab is integer-valued and every
    partial sum stays below 2^24 (the builder asserts it); randn: the reference rounded to f32 and the emulation's sum
    are inside the bound."""
    d = W.build(kind, c)
    slabs = W.emulate(kind, c, d)
    if c["data"] == "int":
        assert float(d["scale"].max()) < 2 ** 24
        W.check_case(kind, c, d["ref"], d)
        W.check_case(kind, c, d["ref"].float(), d)
        W.check_case(kind, c, slabs.sum(0), d)
        assert bool((slabs == slabs.round()).all())
    else:
        assert W.check_case(kind, c, d["ref"].float(), d) <= 1.0
        assert W.check_case(kind, c, slabs.sum(0), d) < 1e-6
    for k, n in enumerate(W.steps(kind, c)):
        if n == 0:
            assert bool((slabs[k] == 0).all())


def test_emulation_blocks_partition_the_pixels():
    for kind, c in W.ALL_CASES:
        seen = sorted((n * c["OH"] + r) * c["OW"] + col for b in range(W.blocks(kind, c))
                      for n, r, col, inside in W.block_positions(kind, c, b) if inside)
        assert seen == list(range(c["N"] * c["OH"] * c["OW"])), c["id"]
        sl = W.slices(kind, c)
        assert sl[0][0] == 0 and max(b1 for _, b1 in sl) == W.blocks(kind, c)
        assert all(sl[k][1] == sl[k + 1][0] or sl[k + 1][1] == sl[k + 1][0] for k in range(len(sl) - 1)), c["id"]


# ---- planted defects ---------------------------------------------------------------------------------------------------

def caught(defect, data):
    """ids of the table cases of either kernel whose check fails with the defect planted."""
    out = {"halo": [], "row": []}
    for kind, c in W.ALL_CASES:
        if c["data"] != data:
            continue
        d = W.build(kind, c)
        try:
            W.check_case(kind, c, W.emulate(kind, c, d, defect).sum(0), d)
        except AssertionError as e:
            assert "differ from the exact sum" in str(e) or "outside the bound" in str(e)
            out[kind].append(c["id"])
    return out


@pytest.mark.parametrize("defect", W.DEFECTS)
def test_planted_defect_fails_the_int_equality(defect):
    got = caught(defect, "int")
    assert got["halo"] and got["row"], (defect, got)


@pytest.mark.parametrize("defect", ["prev_image_row", "prev_row_pixel"])
def test_planted_read_of_a_neighbour_fails_the_randn_bound(defect):
    got = caught(defect, "randn")
    assert got["halo"] and got["row"], (defect, got)
    if defect == "prev_row_pixel":                        # every image wider than one pixel column has such a pixel
        n = {k: len(of(k, "randn")) for k in W.KINDS}
        assert all(len(got[k]) == n[k] for k in W.KINDS), got


def test_equality_report_names_the_tap_and_element():
    kind, c = "halo", W.WH_CASES[4]
    d = W.build(kind, c)
    got = d["ref"].clone()
    got[5, 6, 7] += 1
    got[9, 6, 1] = float("nan")
    with pytest.raises(AssertionError, match=r"2 of .* per tap \[0, 0, 0, 0, 0, 0, 2, 0, 0\]; first at \(a 5, tap 6, b 7\)"):
        W.assert_equal_int(got, d["ref"])


# ---- the restated geometry -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import sfv_amd
    return sfv_amd._lib


@pytest.mark.parametrize("kind,c", W.ALL_CASES, ids=CASE_IDS)
def test_geometry_equals_the_library_queries(lib, kind, c):
    N, OH, OW, Ca, Cb = c["N"], c["OH"], c["OW"], c["Ca"], c["Cb"]
    name = f"rbvae_wgrad3x3s2_{kind}"
    assert lib.query(name + "_ok", 1, N, OH, OW, Ca, Cb) == 1
    assert lib.query(name + "_ok", 0, N, OH, OW, Ca, Cb) == 0                    # f32 is rbvae_wgrad_gemm's
    unit = W.CH_UNIT[kind]
    assert lib.query(name + "_ok", 1, N, OH, OW, Ca + unit // 2, Cb) == 0
    assert lib.query(name + "_ok", 1, N, OH, OW, Ca, unit // 2) == 0
    nblk = lib.query(name + "_blocks", N, OH, OW)
    geo = W.wh_geometry(c) if kind == "halo" else W.wr_geometry(c)
    assert nblk == geo["nblk"] == W.blocks(kind, c)
    assert 1 <= c["ks"] <= nblk
    assert sum(W.steps(kind, c)) == nblk and len(W.steps(kind, c)) == c["ks"]
    if kind == "halo":
        assert max(W.steps(kind, c)) == geo["per"]
        assert geo["grid"] % 8 == 0 and geo["grid"] >= (Ca // 64) * (Cb // 64) * c["ks"]
    else:
        st = W.steps(kind, c)
        assert set(st) <= {geo["base"], geo["base"] + 1} and st == sorted(st, reverse=True) and min(st) >= 1
        assert geo["grid"] % 8 == 0 and 0 <= geo["grid"] - geo["items"] < 8
    # operand layout the ABI asks for: 16-byte aligned column slices of rows with ld % 8 == 0
    assert c["lds"] % 8 == 0 and c["ldg"] % 8 == 0 and c["col_off_s"] % 8 == 0 and c["col_off_g"] % 8 == 0
    assert c["lds"] >= c["col_off_s"] + Ca and c["ldg"] >= c["col_off_g"] + Cb
    assert N * OH * OW <= 1024 and W.k_model(kind, c) <= 1024


# ---- the tables reach every arm --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("data", ["int", "randn"])
def test_halo_cases_reach_every_arm(data):
    cs = of("halo", data)
    geo = [W.wh_geometry(c) for c in cs]
    # ring of four and the four-block unrolled loop: 0 (an empty slice), every residue mod 4, two and more iterations
    assert {s for c in cs for s in W.steps("halo", c)} >= set(range(11))
    assert any(g["over_bottom"] for g in geo) and any(g["over_right"] for g in geo)
    assert any(g["over_bottom"] and g["over_right"] for g in geo) and any(g["sub_block"] for g in geo)
    assert any(c["N"] == 1 and c["OH"] == 1 and c["OW"] == 1 for c in cs)
    # XCD groups: K-slices 8.. in the second group, 16.. in the third, empty trailing slices inside a group
    assert {g["groups"] for g in geo} >= {1, 2, 3}
    assert {c["ks"] for c in cs} >= {1, 2, 3, 5, 9, 11, 17}
    assert any(c["ks"] > 8 and 0 in W.steps("halo", c)[8:] for c in cs)
    assert any(g["grid"] > (c["Ca"] // 64) * (c["Cb"] // 64) * c["ks"] for c, g in zip(cs, geo))
    assert {c["Ca"] // 64 for c in cs} >= {1, 2, 4} and {c["Cb"] // 64 for c in cs} >= {1, 2, 4}
    assert any(c["Ca"] != c["Cb"] for c in cs)
    roles_and_padding(cs)


@pytest.mark.parametrize("data", ["int", "randn"])
def test_row_cases_reach_every_arm(data):
    cs = of("row", data)
    for W_ in (8, 4):
        sub = [(c, W.wr_geometry(c)) for c in cs if W.wr_geometry(c)["W"] == W_]
        assert sub, W_
        RB = 64 // W_
        assert any(c["OH"] == 1 for c, g in sub)
        assert any(c["OH"] < RB and g["rbmod"] == 0 for c, g in sub)
        assert any(1 < c["OH"] < RB and g["rbmod"] != 0 for c, g in sub)
        assert any(c["OH"] > RB and g["top_inside"] for c, g in sub)                 # top set by p_r0 + RB > OH
        assert any(g["short_last"] for c, g in sub) and any(not g["short_last"] for c, g in sub)
        assert any(g["over_right"] for c, g in sub) and any(not g["over_right"] for c, g in sub)
        assert any(g["nstrip"] > 1 for c, g in sub) and any(g["span"] >= 2 for c, g in sub)
        assert any(g["rem"] != 0 for c, g in sub)                                    # unequal balanced slices
        assert {c["Ca"] // 128 for c, g in sub} >= {1, 2} and {c["Cb"] // 128 for c, g in sub} >= {1, 2}
    geo = [W.wr_geometry(c) for c in cs]
    # ring of three: 1 and 2 steps (no steady state), every residue mod 3 beyond
    assert {s for c in cs for s in W.steps("row", c)} >= set(range(1, 9))
    assert max(g["span"] for g in geo) == 16 and {g["span"] for g in geo} >= {1, 2, 3, 4, 7, 16}
    assert {g["items"] for g in geo} >= {3, 6, 9, 12, 15, 18, 21, 27, 48, 60}
    assert any(g["items"] % 8 for g in geo) and any(g["items"] % 8 == 0 for g in geo)
    assert any(c["ks"] == g["nblk"] and c["ks"] > 1 for c, g in zip(cs, geo))
    assert any(c["Ca"] != c["Cb"] for c in cs)
    roles_and_padding(cs)


def roles_and_padding(cs):
    assert {c["role"] for c in cs} == {"conv", "deconv"}
    padded = [c for c in cs if c["col_off_s"] or c["col_off_g"]]
    assert len(cs) // 4 <= len(padded) <= len(cs) // 2
    assert all(c["lds"] > c["Ca"] + c["col_off_s"] and c["ldg"] > c["Cb"] + c["col_off_g"] and c["col_off_s"] and
               c["col_off_g"] for c in padded)                                       # sentinels on both sides
    assert {c["role"] for c in padded} == {"conv", "deconv"}
    assert all(c["lds"] == c["Ca"] and c["ldg"] == c["Cb"] for c in cs if c not in padded)


def test_each_shape_has_an_int_and_a_randn_case_of_both_roles():
    for kind in W.KINDS:
        by = {}
        for c in W.TABLES[kind]:
            by.setdefault((c["N"], c["OH"], c["OW"], c["Ca"], c["Cb"], c["ks"]), []).append(c)
        assert all({c["data"] for c in v} == {"int", "randn"} and {c["role"] for c in v} == {"conv", "deconv"}
                   for v in by.values())
    assert len(set(CASE_IDS)) == len(CASE_IDS)
