"""The halo checker terms of tests/_bounds.py and the case tables of tests/_halo_cases.py without a GPU: exact float64
results pass every check, each single defect of a halo kernel fails one, the staged-operand term is not loose, and the
cases reach every kernel instance and mode the restated dispatch has."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import _bounds as B
import _halo_cases as H

BF, F32 = torch.bfloat16, torch.float32


def conv_case(dtype="bf16", N=2, IH=10, IW=18, Kc=64, Nout=128, pad=(1, 1), gn=1, swish=1, bias=1, stats_cg=16):
    return H.ch(f"cpu_{dtype}_{N}_{IH}_{IW}_{pad}_{gn}{swish}", dtype, N, IH, IW, Kc, Nout, pad=pad, bias=bias, gn=gn,
                swish=swish, stats_cg=stats_cg)


def conv_check(c, d, got):
    return B.check(got, d["ref"], d["S"], out_dtype=H.TDT[c["dtype"]], K=d["K"], pre=d["pre"], nhw=d["nhw"],
                   S_in=d["S_in"], u_in=d["u_in"], what=c["id"])


def gn_conv(c, d, a):
    """float64 conv of a given staged operand a [N][Kc][IH][IW] (+ bias), as rows."""
    y = B.rows(F.conv2d(a, d["w"].double(), None, padding=c["pad"]))
    return y + d["bias"].double() if d["bias"] is not None else y


def _rejects(fn, match="outside the bound"):
    with pytest.raises(AssertionError, match=match):
        fn()


# ---- exact results pass -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("pad", [(1, 1), (0, 0), (2, 2), (1, 0)])
def test_exact_and_rounded_operand_conv_pass(dtype, pad):
    """ref rounded to the storage type passes; so does the kernel's own model: the staged operand rounded to the
    storage type, the conv exact, the sum rounded once."""
    c = conv_case(dtype, pad=pad, Kc=64 if dtype == "bf16" else 32)
    d = H.ch_build(c)
    tdt = H.TDT[dtype]
    conv_check(c, d, d["ref"].to(tdt))
    a, _ = B.staged_operand(d["x"], d["scale"], d["shift"], c["swish"])
    conv_check(c, d, gn_conv(c, d, a.to(tdt).double()).to(tdt))


def test_every_table_case_reference_passes_itself():
    for c in H.CH_CASES:
        d = H.ch_build(c)
        conv_check(c, d, d["ref"].to(H.TDT[c["dtype"]]))
    for c in H.DH_CASES:
        d = H.dh_build(c)
        B.check(d["ref"].to(H.TDT[c["dtype"]]), d["ref"], d["S"], out_dtype=H.TDT[c["dtype"]], K=d["K"],
                scale=d["scale"], nhw=d["nhw"])


# ---- GroupNorm staging defects --------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_groupnorm_on_a_padding_pixel_is_caught(dtype):
    """padding pixels must contribute 0, not swish(0 * scale + shift)"""
    c = conv_case(dtype, Kc=64 if dtype == "bf16" else 32)
    d = H.ch_build(c)
    ph, pw = c["pad"]
    xp = F.pad(d["x"].double(), (pw, pw, ph, ph))                       # zeros first, GroupNorm after: the defect
    a, _ = B.staged_operand(xp, d["scale"], d["shift"], c["swish"])
    c0 = dict(c, pad=(0, 0))
    got = gn_conv(c0, d, a).to(H.TDT[dtype])
    _rejects(lambda: conv_check(c, d, got))


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_scale_shift_of_the_next_image_is_caught(dtype):
    c = conv_case(dtype, N=3, Kc=64 if dtype == "bf16" else 32)
    d = H.ch_build(c)
    a, _ = B.staged_operand(d["x"], d["scale"].roll(-1, 0), d["shift"].roll(-1, 0), c["swish"])
    _rejects(lambda: conv_check(c, d, gn_conv(c, d, a).to(H.TDT[dtype])))


@pytest.mark.parametrize("dtype,swish", [("bf16", 0), ("bf16", 1), ("f32", 1)])
def test_operand_error_of_four_u_in_is_caught(dtype, swish):
    """a relative operand error of 4 u_in on every element, signed to add up in output channel 0, exceeds the bound:
    the u_in S_in term is not loose.  (One u_in of the same error passes.)  f32 without swish is not among the cases:
    there u_in = 2^-24 sits below c_acc, which bounds that case."""
    c = conv_case(dtype, Kc=64 if dtype == "bf16" else 32, swish=swish, bias=0)
    d = H.ch_build(c)
    w = d["w"].double()
    sgn = torch.sign(w[0].sum((1, 2)))                                  # channel 0: one sign per input channel ...
    w[0] = w[0].abs() * sgn[:, None, None]
    d2 = dict(d, w=w)
    a, _ = B.staged_operand(d["x"], d["scale"], d["shift"], swish)
    ref, S = B.ref_and_scale("conv2d", a, w, padding=c["pad"])
    d2.update(ref=B.rows(ref), S=B.rows(S), S_in=B.rows(S))
    pert = sgn[None, :, None, None] * torch.sign(a)                     # ... so that every term's error has one sign
    for k, fails in ((4, True), (1, False)):
        got = gn_conv(c, d2, a * (1 + k * d["u_in"] * pert))
        if fails:
            _rejects(lambda: conv_check(c, d2, got.to(H.TDT[dtype])))
        else:
            conv_check(c, d2, got)


# ---- deconv: one tap missing at the last output column of one parity class ------------------------------------------

@pytest.mark.parametrize("c", [H.DH_CASES[0], H.DH_CASES[5], H.DH_CASES[10]], ids=lambda c: c["id"])
def test_deconv_missing_tap_at_last_column_is_caught(c):
    d = H.dh_build(c)
    tdt, (N, OH, OW) = H.TDT[c["dtype"]], d["nhw"]
    w = d["w"].double().clone()
    w[:, :, 1, 2] = 0                          # class (ch 0, cw 1): rows 2a, columns 2b + 1; tap (1, 2) reads b
    miss = B.rows(F.conv_transpose2d(d["x"].double(), w, None, stride=2, padding=1, output_padding=1))
    full = B.rows(F.conv_transpose2d(d["x"].double(), d["w"].double(), None, stride=2, padding=1, output_padding=1))
    p = torch.arange(N * OH * OW)
    at = ((p // OW % OH) % 2 == 0) & (p % OW == OW - 1)
    got = d["ref"].clone()
    pre = full.clone()
    pre[at] = miss[at]
    if c["form"] == "forward":
        pre = (pre + d["bias"].double()).clamp_min(0) * d["scale"] * d["keep"]
    else:
        pre = pre * d["scale"] * (d["gate"] > 0)
    got[at] = pre[at]
    assert not torch.equal(got, d["ref"])
    _rejects(lambda: B.check(got.to(tdt), d["ref"], d["S"], out_dtype=tdt, K=d["K"], scale=d["scale"], nhw=d["nhw"]))


def test_deconv_colsum_rows_pin_the_tile_and_class():
    """the exact per-row sums pass; the same sums with two classes exchanged, or a tile's rows moved to the next tile,
    fail (what a total over all rows cannot see)"""
    c = H.DH_CASES[5]
    d = H.dh_build(c)
    stored = d["ref"].to(H.TDT[c["dtype"]])
    want, bnd = H.dh_colsum_ref(c, stored)
    assert bool(((want.float().double() - want).abs() <= bnd).all())
    swapped = want.clone().reshape(-1, 4, want.shape[1])[:, [1, 0, 2, 3]].reshape(want.shape)
    assert not bool(((swapped - want).abs() <= bnd).all())
    moved = want.clone()
    moved[4:8] += moved[0:4]
    moved[0:4] = 0
    assert torch.allclose(moved.sum(0), want.sum(0))
    assert not bool(((moved - want).abs() <= bnd).all())


# ---- statistics defects ---------------------------------------------------------------------------------------------

def stats_case(cg=16):
    c = conv_case("bf16", N=2, IH=22, IW=40, Nout=128, stats_cg=cg)
    d = H.ch_build(c)
    stored = d["ref"].to(BF)
    OH, OW, tr, tc, mtiles, _ = H.ch_geometry(c)
    return c, stored, H.ch_tile_of_rows(c), mtiles


def exact_stats(stored, tile, mtiles, cg):
    mean, m2 = H.tile_stats_ref(stored, tile, mtiles, cg)[:2]
    return torch.stack([mean, m2], -1).reshape(-1, 2)


@pytest.mark.parametrize("cg", [16, 32, 64, 128])
def test_exact_statistics_pass_and_layout_is_pinned(cg):
    c, stored, tile, mtiles = stats_case(cg)
    got = exact_stats(stored, tile, mtiles, cg)
    H.check_tile_stats(got.float(), stored, tile, mtiles, cg)
    # the layout: slot mtile * (Nout / cg) + group holds the stats of that tile's rows and channels
    G = 128 // cg
    for t, gi in ((0, 0), (mtiles - 1, G - 1), (3, G // 2)):
        v = stored.double()[tile == t][:, gi * cg:(gi + 1) * cg]
        assert torch.allclose(got[H.stats_slot(t, gi, 128, cg)], torch.stack([v.mean(), ((v - v.mean()) ** 2).sum()]))


def test_ragged_tile_counted_as_full_is_caught():
    c, stored, tile, mtiles = stats_case()
    got = exact_stats(stored, tile, mtiles, 16).reshape(mtiles, -1, 2)
    npix = torch.bincount(tile, minlength=mtiles)
    t = int(torch.nonzero(npix < 256)[0])                      # a ragged tile: its missing pixels counted as zeros
    v = stored.double()[tile == t].reshape(-1, 8, 16)
    full = torch.cat([v, torch.zeros(256 - v.shape[0], 8, 16, dtype=torch.float64)])
    m = full.mean((0, 2))
    got[t, :, 0], got[t, :, 1] = m, ((full - m[None, :, None]) ** 2).sum((0, 2))
    _rejects(lambda: H.check_tile_stats(got.reshape(-1, 2).float(), stored, tile, mtiles, 16), "tile statistics")


@pytest.mark.parametrize("cg", [16, 64])
def test_statistics_group_shifted_by_one_channel_is_caught(cg):
    c, stored, tile, mtiles = stats_case(cg)
    shifted = stored.roll(-1, 1)
    got = exact_stats(shifted, tile, mtiles, cg)
    _rejects(lambda: H.check_tile_stats(got.float(), stored, tile, mtiles, cg), "tile statistics")


def test_gn_finish_reference_and_bounds():
    """the f64 per-(image, group) mean / rstd of gn_finish_ref are torch's group statistics, and the bounds are finite
    and far below the quantities"""
    c, stored, tile, mtiles = stats_case(16)
    mean, rstd, bm, br = H.gn_finish_ref(stored, tile, c, 16, 1e-6)
    OH, OW = H.ch_geometry(c)[:2]
    x = stored.double().reshape(2, OH, OW, 128).permute(0, 3, 1, 2)
    torch.testing.assert_close(mean, x.reshape(2, 8, -1).mean(-1))
    torch.testing.assert_close(rstd, (x.reshape(2, 8, -1).var(-1, unbiased=False) + 1e-6).rsqrt())
    assert bool((bm < 1e-4).all()) and bool((br < 1e-3 * rstd).all())


# ---- wgrad slabs ----------------------------------------------------------------------------------------------------

def wk_exact(c, pix=None):
    d = H.wk_build(c)
    refs = H.wk_slab_refs(d, pix or H.wk_slice_pixels(c))
    return d, torch.stack([r.float() for r, _ in refs])


@pytest.mark.parametrize("c", H.WK_CASES, ids=[c["id"] for c in H.WK_CASES])
def test_exact_slabs_pass(c):
    d, got = wk_exact(c)
    H.check_slabs(got, d, c)


@pytest.mark.parametrize("i", [0, 5, 7])
def test_block_moved_to_the_next_k_slice_is_caught(i):
    c = H.WK_CASES[i]
    sl = H.wk_slices(c)
    k = next(k for k in range(len(sl) - 1) if sl[k][1] > sl[k][0] and sl[k + 1][1] > sl[k + 1][0])
    pix = H.wk_slice_pixels(c)
    last = H.wk_block_pixels(c, sl[k][1] - 1)
    pix[k], pix[k + 1] = pix[k][:-len(last)], last + pix[k + 1]
    d, got = wk_exact(c, pix)
    _, exact = wk_exact(c)
    assert torch.allclose(got.double().sum(0), exact.double().sum(0), atol=1e-3)
    _rejects(lambda: H.check_slabs(got, d, c))


def test_empty_k_slice_left_nan_is_caught():
    c = H.WK_CASES[0]
    sl = H.wk_slices(c)
    k = next(k for k, (b0, b1) in enumerate(sl) if b1 == b0)
    d, got = wk_exact(c)
    got[k] = float("nan")
    _rejects(lambda: H.check_slabs(got, d, c), "not zero")


def test_slices_partition_the_pixels():
    for c in H.WK_CASES:
        pix = H.wk_slice_pixels(c)
        flat = sorted(p for s in pix for p in s)
        assert flat == list(range(c["N"] * c["OH"] * c["OW"])), c["id"]


# ---- the tables reach every instance and mode -------------------------------------------------------------------------

def test_conv_cases_reach_every_dtype_gn_swish_stats_variant():
    want = set()
    for d in ("f32", "bf16"):
        for mode, st, kern in itertools.product(("plain", "gn", "gn_swish"), (False, True),
                                                ("conv_halo_k",) if d == "f32" else ("conv_halo_k", "conv_halo_ws_k")):
            want.add((d, mode, st, kern))
    got = set()
    for c in H.CH_CASES:
        mode = "gn_swish" if c["gn"] and c["swish"] else "gn" if c["gn"] else "plain"
        for v in H.ch_variants(c):
            got.add((c["dtype"], mode, bool(c["stats_cg"]), H.ch_kernel(c, v)))
    assert want <= got, want - got
    # slices 1 / 2 / 4 / 8, 1 / 2 / 4 output-channel tiles, every padding, stats_cg 16 / 32 / 64 (+ 128, one-tile only)
    for d in ("f32", "bf16"):
        cs = [c for c in H.CH_CASES if c["dtype"] == d]
        assert {c["Kc"] // H.KE[d] for c in cs} >= {1, 2, 4, 8}
        assert {c["Nout"] // 128 for c in cs} >= {1, 2, 4}
        assert {c["pad"] for c in cs} >= {(1, 1), (0, 0), (1, 0), (2, 2), (0, 1)}
        assert {c["stats_cg"] for c in cs} >= {16, 32, 64, 128}
        assert any(H.ch_geometry(c)[:2] == (8, 16) for c in cs)                 # the minimum map
    assert all(H.ch_variants(c) == [1] for c in H.CH_CASES if c["stats_cg"] == 128)
    assert H.ch_kernel(H.CH_BIG, 2) == "conv_halo_ws_k" and H.ch_geometry(H.CH_BIG)[5] >= 512


def test_deconv_cases_reach_every_instance():
    reach = set()
    for d in ("f32", "bf16"):
        for TH in range(1, 48):
            for TW in range(4, 129, 4):
                bm = H.dh_tile_rows(d, 2, TH, TW, H.KE[d], 64)
                if bm:
                    reach.add((d, H.dh_strip_cols(TW), 4 if bm == 128 else 8))
    assert reach == H.DH_REACHABLE
    assert {H.dh_instance(c) for c in H.DH_CASES} == H.DH_REACHABLE
    for d in ("f32", "bf16"):
        cs = [c for c in H.DH_CASES if c["dtype"] == d]
        assert {c["form"] for c in cs} == {"forward", "gradient"}
        assert {c["Nout"] for c in cs} & {64} and max(c["Nout"] for c in cs) >= 192


def test_wgrad_cases_reach_both_row_widths_empty_slices_and_xcd_padding():
    halo = [c for c in H.WK_CASES if c["kind"] == "halo"]
    row = [c for c in H.WK_CASES if c["kind"] == "row"]
    assert {H.wr_width(c["OW"]) for c in row} == {8, 4}
    assert any(b1 == b0 for c in halo for b0, b1 in H.wk_slices(c))                  # empty K-slices
    assert any(H.wh_blocks(1, 18, 13) == 10 and c["ks"] == 7 for c in halo)
    assert any(H.wh_grid(c["Ca"], c["Cb"], c["ks"]) > (c["Ca"] // 64) * (c["Cb"] // 64) * c["ks"] for c in halo)
    assert any(H.wr_grid(c["Ca"], c["Cb"], c["ks"]) > (c["Ca"] // 128) * (c["Cb"] // 128) * 3 * c["ks"] for c in row)
    assert any(64 // H.wr_width(c["OW"]) > c["OH"] or (c["N"] * c["OH"]) % (64 // H.wr_width(c["OW"])) for c in row)
    for cs, unit in ((halo, 64), (row, 128)):
        assert {c["Ca"] // unit for c in cs} >= {1, 2} and {c["Cb"] // unit for c in cs} >= {1, 2}
