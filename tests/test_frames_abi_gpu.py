"""GPU: the four raw-frame entry points of csrc/frames.hip called directly (sfv._lib.call) on the argument sets frames.py
never produces -- row0 > 0, every pointer alignment, tables no resampler makes, the LDS limit, a second trip of the
grid-stride loops -- byte for byte (f32: bit for bit) against tests/_frames_cases.py, whose references
tests/test_frames_abi_cpu.py ties to Pillow and to the torch host pipeline and whose named defects it shows to change bytes
of these very cases.  No tolerances: integer arithmetic and f32 operations in a fixed order.

u8 outputs lie inside 4096 sentinel bytes on each side (_bounds.GuardedBytes) and every case runs twice, with sentinel 0xA5
and with 0x5A: a legitimate byte can equal one sentinel, not both, so two runs equal to the reference with intact bands show
that every byte was written and none outside.  f32 outputs lie in _bounds.GuardedFlat.  bounds and kk lie inside int32 bands
of 0x01010101, so a read past a row's ksize entries or past the table changes bytes.  A refused call must raise and leave
interior and bands sentinel.

The second-trip cases (one frame of 4097 x 4096 = 16 781 312 pixels against 65536 workgroups x 256 threads = 16 777 216) are
built and compared on the device from a 256-entry table computed on the CPU; they run rbvae_u8_to_input mode 0 and
rbvae_perturb_u8 kind 2 with a box across pixel 16 777 216.  Kind 1 shares perturb_k's loop and is not run at this size (its
noise alone is 201 MB).

Measured on one MI355X: 55 tests.  Horizontal pass: all 28 cases byte-equal twice (the 16 pointer alignments, out_w 1 / 255 /
256 / 257 / 300, in_w 1, N 3, four boxed cases with row0 19 .. 116, the synthetic table) and the 10921 -> 10921 row, the
largest LDS size launched: 32768 + 32768 = 65536 bytes; 10921 -> 10922 (65540 bytes) is refused with RBVAE_E_UNSUPPORTED, so
the limit in the entry point and the header's sentence stand.  Vertical pass: 13 cases; by the entry point's rule the vector
path serves W4-in0-out0, W344 (its second workgroup 8 bytes), boxed3 (192 row bytes) and synthetic-W4, the scalar path
W4-in1-out0, W4-in0-out2, W5, W87 (second workgroup 5 bytes), boxed0 / 1 / 2 / 4 and synthetic-W5.  Twelve were byte-equal at
once; synthetic-W4 was not: 12 of 408 bytes differed, bytes 2 and 3 of every dword of the output rows whose taps all lie
outside the source, holding whatever an earlier kernel had left in a register (0xA5, 0x5A, 0x01).  The compiler had paired two
of the four clipped bytes into v_ashr_pk_u8_i32, which keeps the upper half of its destination, and that destination is never
written when no tap is taken.  Pillow's tables always take a tap, so no earlier test could see it; resample_v_k now keeps the
four bytes apart and all 13 cases are byte-equal twice, the two runs bit-equal.  perturb_u8: 6 cases byte-equal twice;
u8_to_input: both modes bit-equal; the two 16 781 312-pixel second-trip cases equal on the device; 22 + 18 refused calls raised
and wrote nothing; the three out= calls equal the calls without out.  Scratch builds of the kernel with one defect each were
told apart: resample_v_k without "- row0" fails 12 vertical cases, resample_h_k reading row r instead of row0 + r fails 27
horizontal cases (the counts test_frames_abi_cpu.py predicts), resample_v_k without its out-of-range `continue` fails the two
synthetic cases.  The module takes 2.5 s; the slowest case is the first (0.2 s, it loads the library), the LDS-limit test
0.03 s and each second-trip test 0.02 s.
"""
import numpy as np
import pytest
import torch

import _bounds as B
import _frames_cases as C
import sfv_amd as sfv

pytestmark = pytest.mark.gpu

B.SENTINEL.setdefault(torch.uint8, (torch.uint8, 0xA5))
SENTINELS = (0xA5, 0x5A)
TABLE_GUARD = 1024
call = sfv._lib.call


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _table(a):
    """int32 table inside bands of 0x01010101 -> (buffer, interior)"""
    a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    buf = torch.full((TABLE_GUARD + a.size + TABLE_GUARD,), C.TABLE_GUARD_WORD, dtype=torch.int32, device="cuda")
    buf[TABLE_GUARD:TABLE_GUARD + a.size] = _dev(a)
    return buf, buf[TABLE_GUARD:TABLE_GUARD + a.size]


def _flat_bands_intact(g, what):
    """assert_guards' band check for a GuardedFlat, on the device"""
    ib, pat = B.SENTINEL[g.dtype]
    bits = g.buf.view(ib).view(-1)
    assert bool((bits[:g.g] == pat).all()) and bool((bits[g.g + g.rows:] == pat).all()), f"{what}: a write outside the output"


# ---- rbvae_resample_u8 ---------------------------------------------------------------------------------------------------

def _resample(c, sentinel):
    x = c["x"]
    N, in_h, in_w, _ = x.shape
    out_w = in_w if c["vertical"] else c["bounds"].shape[0]
    xin = B.GuardedBytes(x.size, sentinel, c["in_off"]).fill(_dev(x))
    out = B.GuardedBytes(N * c["out_h"] * out_w * 3, sentinel, c["out_off"])
    assert xin.view.data_ptr() % 4 == c["in_off"] and out.view.data_ptr() % 4 == c["out_off"]
    (bb, b), (kb, k) = _table(c["bounds"]), _table(c["kk"])
    call("rbvae_resample_u8", xin.view, out.view, N, in_h, in_w, c["out_h"], out_w, c["vertical"], c["row0"], b, k, c["ksize"])
    torch.cuda.synchronize()
    B.assert_byte_bands(out, f"{c['id']} sentinel {sentinel:#x}")
    assert bool((bb[:TABLE_GUARD] == C.TABLE_GUARD_WORD).all()) and bool((kb[-TABLE_GUARD:] == C.TABLE_GUARD_WORD).all())
    return out.view.cpu().numpy().reshape(N, c["out_h"], out_w, 3)


def _check_resample(c):
    ref = C.case_ref(c)
    runs = [_resample(c, s) for s in SENTINELS]
    for s, got in zip(SENTINELS, runs):
        bad = np.argwhere(got != ref)
        assert bad.shape[0] == 0, (f"{c['id']} sentinel {s:#x}: {bad.shape[0]} of {ref.size} bytes differ; first at (n, row, x, c) = "
                                   f"{tuple(bad[0])}: got {got[tuple(bad[0])]}, ref {ref[tuple(bad[0])]}")
    assert np.array_equal(runs[0], runs[1])
    return ref


@pytest.mark.parametrize("c", C.horizontal_cases(), ids=[c["id"] for c in C.horizontal_cases()])
def test_resample_horizontal_byte_equal_and_guarded(c):
    ref = _check_resample(c)
    N, in_h, in_w, _ = c["x"].shape
    print(f"\nresample h {c['id']}: {N} x {in_h} x {in_w} rows {c['row0']}..{c['row0'] + c['out_h']} -> {ref.shape[2]} px, ksize "
          f"{c['ksize']}, in & 3 = {c['in_off']}, out & 3 = {c['out_off']}: {ref.size} bytes equal twice, bands intact")


@pytest.mark.parametrize("c", C.vertical_cases(), ids=[c["id"] for c in C.vertical_cases()])
def test_resample_vertical_byte_equal_and_guarded(c):
    ref = _check_resample(c)
    N, in_h, W, _ = c["x"].shape
    print(f"\nresample v {c['id']}: {N} x {in_h} x {W} ({3 * W} row bytes, {c['path']} path) row0 {c['row0']} -> {c['out_h']} rows, "
          f"ksize {c['ksize']}: {ref.size} bytes equal twice, two runs bit-equal, bands intact")


def test_resample_lds_limit_launches_at_65536_and_refuses_the_next_size():
    c = C.lds_case()
    in_w = c["x"].shape[2]
    ref = _check_resample(c)
    print(f"\nresample h {c['id']}: {in_w} -> {ref.shape[2]} px, 32768 + 32768 = 65536 bytes of LDS: {ref.size} bytes equal twice")
    tab = C._rc(in_w, in_w + 1, "bilinear")
    (_, b), (_, k) = _table(tab[0]), _table(tab[1])
    xin = _dev(c["x"])
    for s in SENTINELS:
        out = B.GuardedBytes(3 * (in_w + 1), s)
        with pytest.raises(RuntimeError, match="LDS"):
            call("rbvae_resample_u8", xin, out.view, 1, 1, in_w, 1, in_w + 1, 0, 0, b, k, tab[1].shape[1])
        torch.cuda.synchronize()
        B.assert_bytes_untouched(out, f"{in_w} -> {in_w + 1}")
    print(f"resample h {in_w} -> {in_w + 1} px (65540 bytes of LDS): RBVAE_E_UNSUPPORTED, nothing written")


# ---- rbvae_perturb_u8 / rbvae_u8_to_input ----------------------------------------------------------------------------------

def _perturb(c, sentinel):
    x = c["x"]
    N, H, W, _ = x.shape
    out = B.GuardedBytes(x.size, sentinel)
    noise = None if c["noise"] is None else _dev(c["noise"])
    boxes = None if c["boxes"] is None else _dev(c["boxes"])
    call("rbvae_perturb_u8", _dev(x), out.view, N, H, W, c["kind"], noise, float(c["std"]), float(c["mean"]), boxes)
    torch.cuda.synchronize()
    B.assert_byte_bands(out, f"{c['id']} sentinel {sentinel:#x}")
    return out.view.cpu().numpy().reshape(x.shape)


@pytest.mark.parametrize("c", C.perturb_cases(), ids=[c["id"] for c in C.perturb_cases()])
def test_perturb_byte_equal_and_guarded(c):
    ref = C.perturb_case_ref(c)
    for s in SENTINELS:
        got = _perturb(c, s)
        bad = np.argwhere(got != ref)
        assert bad.shape[0] == 0, (f"{c['id']} sentinel {s:#x}: {bad.shape[0]} of {ref.size} bytes differ; first at (n, y, x, c) = "
                                   f"{tuple(bad[0])}: got {got[tuple(bad[0])]}, ref {ref[tuple(bad[0])]}")
    print(f"\nperturb {c['id']}: kind {c['kind']}, {c['x'].shape[0]} x {c['x'].shape[1]} x {c['x'].shape[2]}: {ref.size} bytes equal "
          f"twice, bands intact")


@pytest.mark.parametrize("mode", [0, 1])
def test_u8_to_input_bit_equal_and_guarded(mode):
    x = C.to_input_frames()
    N, H, W, _ = x.shape
    ref = C.to_input_ref(x, mode)
    out = B.GuardedFlat(ref.size, torch.float32)
    call("rbvae_u8_to_input", _dev(x), out.view, N, H, W, mode)
    torch.cuda.synchronize()
    B.assert_guards(out, f"u8_to_input mode {mode}")
    got = out.view.cpu().numpy().reshape(ref.shape)
    assert np.array_equal(got.view(np.int32), ref.view(np.int32))
    print(f"\nu8_to_input mode {mode}: {N} x {H} x {W}, all 256 byte values: {ref.size} f32 bit-equal, guards intact")


BIG_H, BIG_W = 4096, 4097                   # 16 781 312 pixels: 4096 more than one trip of 65536 x 256 threads


def _big_frame():
    assert BIG_H * BIG_W > 65536 * 256
    return torch.randint(0, 256, (1, BIG_H, BIG_W, 3), dtype=torch.uint8, device="cuda",
                         generator=torch.Generator("cuda").manual_seed(12))


def test_u8_to_input_second_trip_of_the_grid_stride_loop():
    x = _big_frame()
    hw = BIG_H * BIG_W
    out = B.GuardedFlat(3 * hw, torch.float32)
    call("rbvae_u8_to_input", x, out.view, 1, BIG_H, BIG_W, 0)
    torch.cuda.synchronize()
    _flat_bands_intact(out, "u8_to_input 4097 x 4096")
    tab = C.unit_table().cuda()
    got = out.view.view(3, hw).view(torch.int32)
    for ch in range(3):
        want = torch.index_select(tab, 0, x[0, :, :, ch].reshape(-1).int()).view(torch.int32)
        bad = (got[ch] != want).nonzero()
        assert bad.shape[0] == 0, f"channel {ch}: {bad.shape[0]} of {hw} values differ; first at pixel {int(bad[0, 0])}"
    print(f"\nu8_to_input mode 0, 1 x {BIG_H} x {BIG_W}: {3 * hw} f32 bit-equal on the device ({hw - 65536 * 256} pixels in the "
          f"second trip), bands intact")


def test_perturb_second_trip_of_the_grid_stride_loop():
    x = _big_frame()
    s = 16
    box = (0, BIG_H - s, s)                 # rows 4080..4095, columns 0..15: pixels 16 777 215 (x = 0) and 16 777 216 (x = 1) of
    p = (BIG_H - 1) * BIG_W                 # the last row lie inside, one on each side of the first trip's end
    assert p < 65536 * 256 <= p + s - 1
    v = np.arange(256, dtype=np.uint8)
    tab = C.perturb_ref(np.stack([v, v, v], 1).reshape(1, 16, 16, 3), 2, boxes=[(0, 0, 0)])[0, :, :, 0].reshape(-1)
    want = torch.index_select(_dev(tab), 0, x.view(-1).int()).view(x.shape)
    want[0, box[1]:box[1] + s, box[0]:box[0] + s] = 127
    for sent in SENTINELS:
        out = B.GuardedBytes(x.numel(), sent)
        call("rbvae_perturb_u8", x, out.view, 1, BIG_H, BIG_W, 2, None, 0.0, 0.0, torch.tensor([box], dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        B.assert_byte_bands(out, f"perturb 4097 x 4096 sentinel {sent:#x}")
        bad = (out.view != want.view(-1)).nonzero()
        assert bad.shape[0] == 0, f"{bad.shape[0]} of {x.numel()} bytes differ; first at byte {int(bad[0, 0])}"
    print(f"\nperturb kind 2, 1 x {BIG_H} x {BIG_W}, box {box} across pixel {65536 * 256}: {x.numel()} bytes equal twice on the device, "
          f"bands intact")


# ---- refusals ------------------------------------------------------------------------------------------------------------

def _refused(name, outs, exc, *args):
    with pytest.raises(exc):
        call(name, *args)
    torch.cuda.synchronize()
    for g in outs:
        if isinstance(g, B.GuardedBytes):
            B.assert_bytes_untouched(g, name)
        else:
            B.assert_guards_where(g, torch.zeros(g.rows, dtype=torch.bool), name)


def test_resample_refusals_write_nothing():
    x = _dev(C._frames(1, 7, 4, 2))
    tab = C._rc(7, 5, "lanczos")
    (_, b), (_, k) = _table(tab[0]), _table(tab[1])
    ks = tab[1].shape[1]
    n = 0
    for s in SENTINELS:
        out = B.GuardedBytes(2 * 4 * 7 * 3, s)
        good = [x, out.view, 2, 4, 7, 3, 5, 0, 1, b, k, ks]      # in out N in_h in_w out_h out_w vertical row0 bounds kk ksize
        bad = {"in null": {0: None}, "out null": {1: None}, "bounds null": {9: None}, "kk null": {10: None}, "N 0": {2: 0},
               "N 65536": {2: 65536}, "ksize 0": {11: 0}, "row0 + out_h = in_h + 1": {8: 2}, "row0 -1": {8: -1},
               "vertical, in_w != out_w": {7: 1}, "vertical, out_h 65536": {7: 1, 6: 7, 5: 65536}}
        for what, change in bad.items():
            args = list(good)
            for i, v in change.items():
                args[i] = v
            _refused("rbvae_resample_u8", [out], ValueError, *args)
            n += 1
        call("rbvae_resample_u8", *good)                        # and the unchanged arguments are accepted
        torch.cuda.synchronize()
        assert bool((out.view[:2 * 3 * 5 * 3] != s).any())
    print(f"\nresample_u8: {n} refused calls raised ValueError and wrote nothing")


def test_perturb_and_to_input_refusals_write_nothing():
    a = C.perturb_frames()
    N, H, W, _ = a.shape
    x, noise, boxes = _dev(a), _dev(C.noise_for(0.1, 0.0)), _dev(C.perturb_cases()[3]["boxes"])
    n = 0
    for s in SENTINELS:
        out = B.GuardedBytes(a.size, s)
        good = [x, out.view, N, H, W, 1, noise, 0.1, 0.0, boxes]  # in out N H W kind noise std mean boxes
        for change in ({0: None}, {1: None}, {2: 0}, {5: 0}, {5: 3}, {5: 1, 6: None}, {5: 2, 9: None}):
            args = list(good)
            for i, v in change.items():
                args[i] = v
            _refused("rbvae_perturb_u8", [out], ValueError, *args)
            n += 1
    f = B.GuardedFlat(a.size, torch.float32)
    for change in ({0: None}, {1: None}, {2: 0}, {5: 2}):
        args = [x, f.view, N, H, W, 0]
        for i, v in change.items():
            args[i] = v
        _refused("rbvae_u8_to_input", [f], ValueError, *args)
        n += 1
    print(f"\nperturb_u8 / u8_to_input: {n} refused calls raised ValueError and wrote nothing")


# ---- frames.py's out= ---------------------------------------------------------------------------------------------------------

def test_python_layer_out_goes_into_a_guarded_tensor():
    a = C._frames(30, 31, 9, 2)
    x = _dev(a)
    boxes = [(3, 2, 5), (26, 4, 5)]
    jobs = [("resize_u8 horizontal only", (2, 9, 20, 3), lambda o: sfv.resize_u8(x, (20, 9), "lanczos", out=o)),
            ("resize_u8 two passes", (2, 5, 20, 3), lambda o: sfv.resize_u8(x, (20, 5), "lanczos", out=o)),
            ("perturb_u8", (2, 9, 31, 3), lambda o: sfv.perturb_u8(x, "occlusion", boxes=boxes, out=o))]
    for what, shape, run in jobs:
        plain = run(None)
        assert tuple(plain.shape) == shape
        for s in SENTINELS:
            g = B.GuardedBytes(plain.numel(), s)
            res = run(g.view.view(shape))
            torch.cuda.synchronize()
            assert res.data_ptr() == g.view.data_ptr()
            B.assert_byte_bands(g, f"{what} sentinel {s:#x}")
            assert torch.equal(g.view.view(shape), plain), what
        print(f"\n{what} out=: {plain.numel()} bytes equal to the call without out, twice, bands intact")
