"""CPU: the numpy restatement of the raw-frame ABI (tests/_frames_cases.py) tied to Pillow and to the torch host pipeline,
and the proof that the cases test_frames_abi_gpu.py runs can tell a wrong kernel from a right one: every named defect
changes at least one byte of at least one of them.

A contraction of mode 1's 2 * q - 1 is not among the defects: 2 * q is exact, so the fused and the two-step form round the
same real number once and cannot differ (test_two_q_minus_one_cannot_be_contracted_wrongly shows it on all 256 bytes)."""
import numpy as np
import pytest
import torch

import sfv_amd as sfv
import _frames_cases as C
from _frames_ref import add_gaussian_noise, add_occlusion, to_pil_array, to_tensor


def _all_resample_cases():
    return C.horizontal_cases() + [C.lds_case()] + C.vertical_cases()


@pytest.mark.parametrize("i", range(len(C.BOXED)))
def test_boxed_cases_equal_pillow(i):
    """boxed_coeffs + resample_ref (horizontal pass over the rows the vertical pass reads, row0 > 0, then the vertical
    pass) = PIL.Image.resize(size, filter, box=box), byte for byte."""
    pytest.importorskip("PIL")
    from PIL import Image
    from _frames_ref import pil_filter
    d = C.boxed_case(i)
    want = np.asarray(Image.fromarray(d["x"][0]).resize(d["size"], pil_filter(d["filter"]), box=d["box"]))
    assert d["out"].shape[1:] == want.shape
    assert np.array_equal(d["out"][0], want)
    (iw, ih), _, _, _, rows = C.BOXED[i]
    if rows is not None:
        assert d["h"][0] > 0 and d["h"][1] < ih                 # what resize_u8 never passes
    print(f"\nboxed {i}: {iw}x{ih} box {d['box']} -> {d['size']} {d['filter']} equal to Pillow, row0/rows {rows}")


@pytest.mark.parametrize("filt", ["lanczos", "bilinear"])
@pytest.mark.parametrize("a,b", [(67, 29), (45, 90), (1, 4), (97, 256), (10921, 10921)])
def test_boxed_coeffs_without_a_box_are_resample_coeffs(a, b, filt):
    bo, kk = C.boxed_coeffs(a, 0, a, b, filt)
    rb, rk = sfv.resample_coeffs(a, b, filt)
    assert bo.dtype == rb.dtype and kk.dtype == rk.dtype and np.array_equal(bo, rb) and np.array_equal(kk, rk)


def test_int32_precondition_holds_on_every_table():
    """resample_ref asserts |acc| < 2^31 itself; here for every case of the lists, and for the synthetic tables on the
    worst input any u8 frame can be (sum |k| * 255 + 2^21)."""
    n = 0
    for c in _all_resample_cases():
        _, acc = C.case_ref(c, return_acc=True)
        assert int(np.abs(acc).max()) < 2 ** 31, c["id"]
        assert int(np.abs(c["kk"].astype(np.int64)).sum(1).max()) * 255 + (1 << 21) < 2 ** 31, c["id"]
        n += 1
    print(f"\n{n} resample cases inside int32")


def test_synthetic_tables_clip_at_both_ends_and_leave_the_source():
    for c in [c for c in C.horizontal_cases() + C.vertical_cases() if c["id"].startswith("synthetic")]:
        out, acc = C.case_ref(c, return_acc=True)
        v = acc >> C.PREC
        assert int((v < 0).sum()) > 0 and int((v > 255).sum()) > 0, c["id"]
        assert int((out == 0).sum()) > 0 and int((out == 255).sum()) > 0
        first = c["bounds"][:, 0].astype(np.int64) - (c["row0"] if c["vertical"] else 0)
        taps = c["bounds"][:, 1]
        in_size = c["x"].shape[1] if c["vertical"] else c["x"].shape[2]
        assert int(first.min()) < 0 and int((first + np.minimum(taps, c["ksize"])).max()) > in_size
        assert int(taps.max()) > c["ksize"] and int(taps.min()) == 0
        assert int(c["kk"].min()) >= -2 ** 20 and int(c["kk"].max()) <= 2 ** 21


def _differs(cases, ref, defect):
    return [c["id"] for c in cases if not np.array_equal(ref(c), ref(c, defect))]


@pytest.mark.parametrize("defect", C.RESAMPLE_DEFECTS)
def test_every_resample_defect_shows_on_the_gpu_cases(defect):
    hit = _differs(_all_resample_cases(), C.case_ref, defect)
    print(f"\n{defect}: changes bytes of {len(hit)} cases: {hit[:8]}")
    assert hit
    if defect in ("h_ignores_row0", "v_ignores_row0"):          # the boxed cases are there for this
        assert any(i.startswith("boxed") for i in hit)


@pytest.mark.parametrize("defect", C.PERTURB_DEFECTS)
def test_every_perturb_defect_shows_on_the_gpu_cases(defect):
    hit = _differs(C.perturb_cases(), C.perturb_case_ref, defect)
    print(f"\n{defect}: changes bytes of {hit}")
    assert hit


def test_to_input_defect_shows_and_reference_is_true_division():
    x = C.to_input_frames()
    assert len(np.unique(x)) == 256
    for mode in (0, 1):
        a, b = C.to_input_ref(x, mode), C.to_input_ref(x, mode, "times_reciprocal")
        assert not np.array_equal(a.view(np.int32), b.view(np.int32)), mode
    tab = C.unit_table().numpy()
    got = C.to_input_ref(x, 0)
    assert np.array_equal(got.view(np.int32), np.transpose(tab[x], (0, 3, 1, 2)).view(np.int32))


def test_two_q_minus_one_cannot_be_contracted_wrongly():
    q = C.unit_table().numpy()
    two_step = (np.float32(2.0) * q) - np.float32(1.0)
    fused = (2.0 * q.astype(np.float64) - 1.0).astype(np.float32)      # the exact 2q - 1 rounded once = fma(2, q, -1)
    assert np.array_equal(two_step.view(np.int32), fused.view(np.int32))


def test_references_equal_the_torch_host_pipeline():
    """perturb_ref / to_input_ref against _frames_ref's to_tensor, add_gaussian_noise, add_occlusion and to_pil_array."""
    for c in C.perturb_cases():
        got = C.perturb_case_ref(c)
        for j in range(c["x"].shape[0]):
            t = to_tensor(c["x"][j])
            if c["kind"] == 1:
                ref = add_gaussian_noise(t, torch.from_numpy(c["noise"][j:j + 1]), c["std"], c["mean"])
            else:
                ref = add_occlusion(t, c["boxes"][j])
            assert np.array_equal(got[j], to_pil_array(ref)), (c["id"], j)
    x = C.to_input_frames()
    for j in range(x.shape[0]):
        t = to_tensor(x[j])
        assert torch.equal(torch.from_numpy(C.to_input_ref(x, 0)[j]), t)
        assert torch.equal(torch.from_numpy(C.to_input_ref(x, 1)[j]), 2. * t - 1.)
    assert all(len(np.unique(C.all_bytes_frames()[..., ch])) == 256 for ch in range(3))


def test_case_lists_cover_what_the_issue_names():
    h = {c["id"]: c for c in C.horizontal_cases()}
    assert sum(i.startswith("align") for i in h) == 16
    assert {(c["in_off"], c["out_off"]) for c in h.values() if c["id"].startswith("align")} == {(i, o) for i in range(4) for o in range(4)}
    assert all(c["row0"] > 0 and c["out_h"] < c["x"].shape[1] for i, c in h.items() if i.startswith("boxed"))
    lds = C.lds_case()
    assert ((3 * lds["x"].shape[2] + 7) & ~3) + ((3 * lds["bounds"].shape[0] + 7) & ~3) == 65536
    v = {c["id"]: c["path"] for c in C.vertical_cases()}
    assert v["W4-in0-out0"] == "vector" and v["W4-in1-out0"] == "scalar" and v["W4-in0-out2"] == "scalar"
    assert v["W5-in0-out0"] == "scalar" and v["W87-in0-out0"] == "scalar" and v["W344-in0-out0"] == "vector"
    assert sum(i.startswith("boxed") for i in v) == 5
