"""The LDM decoder on the device (csrc/upconv.hip, LDMDecoder): tests/_upconv_cases.py holds the cases, the restated
dispatch and the float64 references, tests/_bounds.py the error model and the guarded buffers, tests/_ldm_decoder_ref.py the
CPU restatement pinned to the reference's own Decoder by tests/golden/ldm_decoder.npz.

  rbvae_upconv_fold         bit-equal to the float32 CPU fold, pad columns zero, guards untouched
  rbvae_upconv3x3_halo      element-wise |got - ref| <= _bounds.bound(K = 4 Kc) against the float64 four-class reference built
                            from the DEVICE's folded weights; outputs inside NaN guard bands, inputs poisoned outside their
                            interior; a dropped tap, swapped classes, an edge row from the wrong side and an unfolded w[1]
                            each put the reference outside the bound; refused shapes return RBVAE_E_UNSUPPORTED and
                            change no byte
  rbvae_gather_gemm         the same cases through the four-class descriptor, the same bound
  rbvae_latent_rows / rbvae_decoded_to_image   byte for byte against torch float32 on the CPU
  rbvae_nearest2x_rows      bit-equal to repeat_interleave on NHWC rows, both types, padded ldi / ldo (NaN / sentinel columns),
                            a second trip of its grid-stride loop, refusals that write nothing (end of this file)
  LDMDecoder                float32, all three upsample forms: both fixture cases within atol = 8 e32, e32 = 3.04e-6 = max
                            |float32 restatement - float64 restatement| over the fixture outputs (test_ldm_decoder_cpu.py
                            measures it; another summation order and the folded weights each cost about one such floor, a
                            wrong tap or class moves outputs by 0.1 - 1); bf16: relative L2 < 5e-2 (the encoder test's gate);
                            decode_u8 = rbvae_decoded_to_image of decode's rows, chunked = unchunked, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import _bounds as B
import _ldm_decoder_ref as DR
import _upconv_cases as U
from _golden import load

pytestmark = pytest.mark.gpu

E32 = 3.04e-6
E_UNSUPPORTED = -3


@pytest.fixture(scope="module")
def lib():
    import sfv_amd
    return sfv_amd._lib


@pytest.fixture(scope="module")
def fixture():
    g = load("ldm_decoder")
    return g, DR.init_params(int(g["meta/seed"]))


def zero_page():
    return torch.zeros(256, dtype=torch.uint8, device="cuda")


def f32_row(t):
    t = t.reshape(1, -1).float()
    return B.poisoned(t, t.shape[1], torch.float32)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def device_fold(lib, dtype, w, Kc):
    """rbvae_upconv_fold into a guarded buffer -> Guarded of rows [Co * 16][Kc]"""
    Co, Ci = w.shape[:2]
    out = B.guarded(Co * 16, Kc, Kc, U.TDT[dtype])
    wg = B.poisoned(w.reshape(Co, -1), Ci * 9, torch.float32)
    lib.call("rbvae_upconv_fold", U.DTYPE_ID[dtype], wg.view, out.view, Co, Ci, Kc)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("Co,Ci,Kc", U.FOLD_CASES)
def test_upconv_fold_bit_equal_and_guarded(lib, dtype, Co, Ci, Kc):
    g = torch.Generator().manual_seed(Co + Ci)
    w = torch.randn(Co, Ci, 3, 3, generator=g)
    out = device_fold(lib, dtype, w, Kc)
    B.assert_guards(out, f"upconv_fold {dtype} {Co} {Ci} {Kc}")
    want = DR.fold_upconv(w, Kc=Kc).to(U.TDT[dtype])
    got = out.out.cpu().reshape(Co, 16, Kc)
    assert torch.equal(bits(got), bits(want))
    assert bool((got[:, :, Ci:] == 0).all())


def halo_operands(c, d):
    tdt = U.TDT[c["dtype"]]
    return dict(A=B.poisoned(d["A"], c["lda"], tdt), bias=f32_row(d["bias"]) if d["bias"] is not None else None,
                addend=B.poisoned(d["addend"], c["ldo"], tdt) if d["addend"] is not None else None)


def run_halo(lib, c, ops, wf, out):
    lib.call("rbvae_upconv3x3_halo", U.DTYPE_ID[c["dtype"]], ops["A"].view, wf.view, out.view, ops["bias"] and ops["bias"].view,
             ops["addend"] and ops["addend"].view, zero_page(), c["N"], c["h"], c["w"], c["Kc"], c["Nout"], c["lda"], c["ldo"])
    torch.cuda.synchronize()


def run_gather(lib, c, ops, wf, out):
    desc = DR.upconv_class_desc()
    cd = (ctypes.c_int * len(desc))(*desc)
    h, w = c["h"], c["w"]
    lib.call("rbvae_gather_gemm", U.DTYPE_ID[c["dtype"]], ops["A"].view, wf.view, out.view, ops["bias"] and ops["bias"].view,
             None, None, ops["addend"] and ops["addend"].view, zero_page(), c["N"], h, w, h, w, 1, 2 * h, 2 * w, 2, c["Kc"],
             c["Nout"], c["lda"], c["ldo"], 16, 4, ctypes.addressof(cd), 0, 0, 0.0, 1.0, 0, None, None)
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", U.UC_CASES, ids=[c["id"] for c in U.UC_CASES])
def test_upconv3x3_halo_bounded_guarded_and_defects_caught(lib, c):
    tdt, N, h, w, Kc, Nout = U.TDT[c["dtype"]], c["N"], c["h"], c["w"], c["Kc"], c["Nout"]
    assert U.uc_ok(c["dtype"], N, h, w, Kc, Nout)
    assert lib.query("rbvae_upconv3x3_halo_ok", U.DTYPE_ID[c["dtype"]], N, h, w, Kc, Nout) == 1
    d = U.uc_build(c)
    ops = halo_operands(c, d)
    wf = device_fold(lib, c["dtype"], d["w"], Kc)
    wf_cpu = wf.out.cpu().reshape(Nout, 16, Kc)
    ref, S, pre = U.uc_reference(c, d, wf_cpu)
    for form, run in (("halo", run_halo), ("gather", run_gather)):
        out = B.guarded(N * 4 * h * w, c["ldo"], Nout, tdt)
        run(lib, c, ops, wf, out)
        what = f"{c['id']} {form}"
        B.assert_guards(out, what)
        worst = B.check(out.out, ref, S, out_dtype=tdt, K=d["K"], pre=pre, nhw=d["nhw"], what=what)
        print(f"\nBOUNDS upconv {what} worst |err|/bound = {worst:.3g}")
        if form == "halo":
            got = out.out.cpu()
    # the bound tells every named defect from the kernel's result
    for defect in ("dropped_tap", "swapped_classes", "wrong_edge", "unfolded_w1"):
        rd, Sd, pd = U.uc_reference(c, d, wf_cpu, defect)
        with pytest.raises(AssertionError):
            B.check(got, rd, Sd, out_dtype=tdt, K=d["K"], pre=pd, nhw=d["nhw"], what=defect)


@pytest.mark.parametrize("c", U.GATHER_ONLY, ids=[c["id"] for c in U.GATHER_ONLY])
def test_upconv_gather_form_on_shapes_the_halo_kernel_refuses(lib, c):
    tdt, N, h, w, Kc, Nout = U.TDT[c["dtype"]], c["N"], c["h"], c["w"], c["Kc"], c["Nout"]
    assert not U.uc_ok(c["dtype"], N, h, w, Kc, Nout)
    d = U.uc_build(c)
    ops = halo_operands(c, d)
    wf = device_fold(lib, c["dtype"], d["w"], Kc)
    ref, S, pre = U.uc_reference(c, d, wf.out.cpu().reshape(Nout, 16, Kc))
    out = B.guarded(N * 4 * h * w, c["ldo"], Nout, tdt)
    run_gather(lib, c, ops, wf, out)
    B.assert_guards(out, c["id"])
    B.check(out.out, ref, S, out_dtype=tdt, K=d["K"], pre=pre, nhw=d["nhw"], what=c["id"])


@pytest.mark.parametrize("shape", U.UC_REFUSED, ids=["-".join(map(str, s)) for s in U.UC_REFUSED])
def test_upconv3x3_halo_refused_shapes_write_nothing(lib, shape):
    dtype, N, h, w, Kc, Nout = shape
    tdt = U.TDT[dtype]
    assert not U.uc_ok(*shape)
    assert lib.query("rbvae_upconv3x3_halo_ok", U.DTYPE_ID[dtype], N, h, w, Kc, Nout) == 0
    A = B.poisoned(torch.randn(N * h * w, Kc), Kc, tdt)
    wf = B.poisoned(torch.randn(Nout * 16, Kc), Kc, tdt)
    out = B.guarded(N * 4 * h * w, Nout, Nout, tdt)
    before = out.buf.clone()
    rc = lib.lib().rbvae_upconv3x3_halo(U.DTYPE_ID[dtype], A.view.data_ptr(), wf.view.data_ptr(), out.view.data_ptr(), None, None,
                                        zero_page().data_ptr(), N, h, w, Kc, Nout, Kc, Nout, lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == E_UNSUPPORTED
    assert torch.equal(bits(out.buf), bits(before))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_latent_rows_byte_for_byte(lib, dtype):
    tdt, Kpad = U.TDT[dtype], U.KE[dtype]
    g = torch.Generator().manual_seed(11)
    N, Z, HW = 3, 4, 35
    z = torch.randn(N, Z, HW, generator=g) * 0.9
    z[0, 0, :4] = torch.tensor([0.18215, -0.18215, 0.0, 3e38])
    want = torch.zeros(N * HW, Kpad, dtype=tdt)
    want[:, :Z] = (1. / 0.18215 * z).permute(0, 2, 1).reshape(N * HW, Z).to(tdt)          # ddpm.py:713, then the storage type
    zg = B.poisoned(z.reshape(N * Z, HW), HW, torch.float32, row_align=4)
    out = B.guarded(N * HW, Kpad, Kpad, tdt)
    lib.call("rbvae_latent_rows", U.DTYPE_ID[dtype], zg.view, out.view, N, Z, HW, Kpad, 0.18215)
    torch.cuda.synchronize()
    B.assert_guards(out, "latent_rows")
    assert torch.equal(bits(out.out), bits(want))


@pytest.mark.parametrize("dtype,ld", [("f32", 12), ("bf16", 24), ("f32", 4), ("bf16", 8)])
def test_decoded_to_image_byte_for_byte(lib, dtype, ld):
    tdt = U.TDT[dtype]
    vals = U.image_values(dtype)                       # [M][3]
    N = 2
    assert vals.shape[0] % N == 0
    HW = vals.shape[0] // N
    rows = B.poisoned(vals, ld, tdt)
    img = B.GuardedFlat(N * 3 * HW, torch.float32)
    guard = 4096
    u8 = torch.full((guard + N * HW * 3 + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    lib.call("rbvae_decoded_to_image", U.DTYPE_ID[dtype], rows.view, ld, img.view, u8[guard:], N, HW)
    torch.cuda.synchronize()
    B.assert_guards(img, "decoded_to_image f32")
    x = vals.float().reshape(N, HW, 3).permute(0, 2, 1).contiguous()           # the decoder's output [N][3][HW]
    assert torch.equal(bits(img.out.reshape(N, 3, HW)), bits(x))
    want = DR.to_u8(x.reshape(N, 3, HW, 1))
    u8c = u8.cpu()
    assert bool((u8c[:guard] == 0xA5).all()) and bool((u8c[guard + N * HW * 3:] == 0xA5).all())
    assert np.array_equal(u8c[guard:guard + N * HW * 3].numpy().reshape(N, HW, 1, 3), want)
    # each output alone leaves the other untouched and gives the same bytes
    u8b = torch.full_like(u8, 0xA5)
    lib.call("rbvae_decoded_to_image", U.DTYPE_ID[dtype], rows.view, ld, None, u8b[guard:], N, HW)
    assert torch.equal(u8b.cpu(), u8c)


def make_decoder(sfv, g, p, dtype, impl, halo_where_covered=True):
    """halo_where_covered: "halo" runs upconv_halo_k on every shape it covers, whatever the product's dispatch rule says"""
    torch.manual_seed(int(g["meta/seed"]))
    m = sfv.LDMDecoder(compute_dtype=dtype, upsample_impl=impl, halo_where_covered=halo_where_covered)
    sd = m.state_dict()
    assert list(sd.keys()) == list(p.keys())
    for k in p:                                        # same construction order => same initial weights
        assert torch.equal(sd[k], p[k]), k
    return m.cuda()


@pytest.mark.parametrize("impl", ["halo", "gather", "unfolded"])
def test_decoder_f32_matches_reference_decoder(fixture, impl):
    import sfv_amd as sfv
    g, p = fixture
    m = make_decoder(sfv, g, p, "f32", impl)
    for tag, (h, w) in (("a", (8, 8)), ("b", (4, 12))):
        z = torch.from_numpy(g[f"z_{tag}"]).cuda()
        out = m.decode(z).cpu().numpy()
        err = float(np.abs(out - g[f"out_{tag}"]).max())
        print(f"\nDECODER f32 {impl} case {tag}: max |err| = {err:.3g} (gate {8 * E32:.3g})")
        forms = [(impl if impl != "halo" or min(h << i, w << i) >= 5 else "gather", h << i, w << i) for i in range(3)]
        assert m.upsample_dispatch == forms, m.upsample_dispatch
        np.testing.assert_allclose(out, g[f"out_{tag}"], atol=8 * E32, rtol=0)
    if impl == "halo":                                 # the 4 x 12 latent's first Upsample took the fallback
        assert m.upsample_dispatch[0] == ("gather", 4, 12) and m.upsample_dispatch[1] == ("halo", 8, 24)
        # the product's own rule: only shapes _upconv_halo_rule names leave the gather form, and never one the kernel refuses
        d = make_decoder(sfv, g, p, "f32", "halo", halo_where_covered=False)
        out = d.decode(z).cpu().numpy()
        np.testing.assert_allclose(out, g["out_b"], atol=8 * E32, rtol=0)
        want = [("halo" if d._upconv_halo_rule(1, 4 << i, 12 << i, 512) and min(4 << i, 12 << i) >= 5 else "gather", 4 << i, 12 << i)
                for i in range(3)]
        assert d.upsample_dispatch == want and want[0][0] == "gather"


@pytest.mark.parametrize("impl", ["halo", "gather", "unfolded"])
def test_decoder_bf16_tracks_reference_decoder(fixture, impl):
    import sfv_amd as sfv
    g, p = fixture
    m = make_decoder(sfv, g, p, "bf16", impl)
    for tag in "ab":
        out = m.decode(torch.from_numpy(g[f"z_{tag}"]).cuda()).cpu().numpy()
        ref = g[f"out_{tag}"]
        rel = float(np.linalg.norm(out - ref) / np.linalg.norm(ref))
        print(f"\nDECODER bf16 {impl} case {tag}: relative L2 = {rel:.3g}")
        assert rel < 5e-2


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_decode_u8_and_chunking_bit_for_bit(lib, fixture, dtype):
    import sfv_amd as sfv
    g, p = fixture
    m = make_decoder(sfv, g, p, dtype, "halo")
    z = torch.cat([torch.from_numpy(g["z_a"]), torch.from_numpy(g["z_a"]).flip(0)[:1] * 0.5]).cuda()      # 3 latents
    full = m.decode(z)
    u8 = m.decode_u8(z)
    assert full.shape == (3, 3, 64, 64) and full.dtype == torch.float32 and u8.shape == (3, 64, 64, 3) and u8.dtype == torch.uint8
    rows = m._rows(z.float().contiguous())
    want = torch.empty_like(u8)
    lib.call("rbvae_decoded_to_image", U.DTYPE_ID[dtype], rows, rows.shape[1], None, want, 3, 64 * 64)
    assert torch.equal(u8, want)
    assert np.array_equal(u8.cpu().numpy(), DR.to_u8(full))                    # ldm_embedding_interpol.py:179-182 on decode's values
    for chunk in (1, 2):
        assert torch.equal(m.decode(z, chunk=chunk), full), chunk
        assert torch.equal(m.decode_u8(z, chunk=chunk), u8), chunk
    buf = torch.zeros(3 * 3 * 64 * 64, device="cuda")
    assert m.decode(z, out=buf).data_ptr() == buf.data_ptr() and torch.equal(buf.view_as(full), full)


def test_checkpoint_keys_and_errors(fixture):
    import sfv_amd as sfv
    g, p = fixture
    m = make_decoder(sfv, g, p, "bf16", "halo")
    # a Stable-Diffusion style checkpoint (first_stage_model.* keys, encoder / loss entries beside the decoder's) loads as is
    sd = {f"first_stage_model.{k}": v + 0.01 for k, v in m.state_dict().items()}
    sd["first_stage_model.encoder.conv_in.weight"] = torch.zeros(3)
    sd["first_stage_model.quant_conv.bias"] = torch.zeros(8)
    sd["first_stage_model.loss.logvar"] = torch.zeros(1)
    m2 = sfv.LDMDecoder(compute_dtype="bf16")
    m2.load_state_dict(sd)
    for k0 in ("decoder.up.3.upsample.conv.weight", "post_quant_conv.bias"):
        assert torch.allclose(m2.state_dict()[k0], m.state_dict()[k0].cpu() + 0.01)
    z = torch.from_numpy(g["z_a"])
    with pytest.raises(RuntimeError):
        m.decode(z)
    with pytest.raises(RuntimeError):
        m.decode_u8(z)
    with pytest.raises(ValueError):
        m.decode(torch.zeros(1, 3, 8, 8, device="cuda"))
    with pytest.raises(ValueError):
        m.decode(torch.zeros(4, 8, 8, device="cuda"))


# ---- rbvae_nearest2x_rows: the "unfolded" baseline's upsampled rows, on their own ------------------------------------------
# Measured on one MI355X: all 36 padded cases and the 1 x 1024 x 1025 x 16 second-trip case bit-equal, padding columns and
# bands untouched, no NaN read; 9 refused calls wrote nothing; each test under 0.2 s.

def _nearest_want(x, N, IH, IW, C):
    """out[(n, 2r+p, 2c+q)] = in[(n, r, c)] on NHWC rows"""
    return x.reshape(N, IH, IW, C).repeat_interleave(2, 1).repeat_interleave(2, 2).reshape(N * 4 * IH * IW, C)


@pytest.mark.parametrize("pad", [(0, 0), (1, 0), (0, 2)], ids=["ld=C", "ldi+16B", "ldo+32B"])
@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("N,IH,IW", [(1, 1, 1), (2, 3, 5), (1, 7, 4)])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_nearest2x_rows_bit_equal_padded_and_guarded(lib, dtype, N, IH, IW, chunks, pad):
    tdt = U.TDT[dtype]
    per = 16 // torch.empty((), dtype=tdt).element_size()         # elements of one 16-byte chunk: 4 f32, 8 bf16
    C, ldi, ldo = chunks * per, (chunks + pad[0]) * per, (chunks + pad[1]) * per
    x = torch.randn(N * IH * IW, C, generator=torch.Generator().manual_seed(N + IH + IW + C)).to(tdt)
    xin = B.poisoned(x, ldi, tdt)                                  # columns C..ldi and the bands are NaN
    out = B.guarded(N * 4 * IH * IW, ldo, C, tdt)                  # columns C..ldo and the bands are sentinel
    lib.call("rbvae_nearest2x_rows", U.DTYPE_ID[dtype], xin.view, out.view, N, IH, IW, C, ldi, ldo)
    torch.cuda.synchronize()
    what = f"nearest2x_rows {dtype} {N} x {IH} x {IW} C {C} ldi {ldi} ldo {ldo}"
    B.assert_guards(out, what)
    got = out.out.cpu()
    assert not bool(torch.isnan(got.float()).any())
    assert torch.equal(bits(got), bits(_nearest_want(x, N, IH, IW, C))), what
    print(f"\n{what}: {got.numel()} elements bit-equal, padding columns and bands untouched")


def test_nearest2x_rows_second_trip_of_the_grid_stride_loop(lib):
    """1 x 1024 x 1025 x 16 f32: 16 793 600 chunks against 65536 workgroups x 256 threads = 16 777 216; 67 MB in, 268 MB out,
    compared on the device."""
    N, IH, IW, C = 1, 1024, 1025, 16
    assert N * 4 * IH * IW * (C // 4) > 65536 * 256
    x = torch.randn(N * IH * IW, C, device="cuda", generator=torch.Generator("cuda").manual_seed(13))
    xin = B.poisoned(x, C, torch.float32)
    out = B.guarded(N * 4 * IH * IW, C, C, torch.float32)
    lib.call("rbvae_nearest2x_rows", U.DTYPE_ID["f32"], xin.view, out.view, N, IH, IW, C, C, C)
    torch.cuda.synchronize()
    pat = B.SENTINEL[torch.float32][1]
    raw = out.buf.view(torch.int32)
    assert bool((raw[:out.g] == pat).all()) and bool((raw[out.g + out.rows:] == pat).all()), "a write outside the output"
    bad = (out.view.view(torch.int32) != _nearest_want(x, N, IH, IW, C).view(torch.int32)).nonzero()
    assert bad.shape[0] == 0, f"{bad.shape[0]} elements differ; first at (row {int(bad[0, 0])}, column {int(bad[0, 1])})"
    print(f"\nnearest2x_rows f32 {N} x {IH} x {IW} C {C}: {out.view.numel()} elements bit-equal on the device, bands untouched")


def test_nearest2x_rows_refusals_write_nothing(lib):
    N, IH, IW = 2, 3, 5
    x = B.poisoned(torch.randn(N * IH * IW, 8), 8, torch.float32)
    out = B.guarded(N * 4 * IH * IW, 8, 8, torch.float32)
    before = out.buf.clone()
    f32 = U.DTYPE_ID["f32"]
    assert 7 not in U.DTYPE_ID.values()
    lib.call("rbvae_nearest2x_rows", f32, x.view, B.guarded(N * 4 * IH * IW, 8, 8, torch.float32).view, N, IH, IW, 8, 8, 8)   # the base is accepted
    refused = {                                                    # dtype in out N IH IW C ldi ldo
        "C not a multiple of the chunk": (f32, x.view, out.view, N, IH, IW, 6, 8, 8),
        "ldi < C": (f32, x.view, out.view, N, IH, IW, 8, 4, 8),
        "ldo not a multiple of 16 bytes": (f32, x.view, out.view, N, IH, IW, 4, 8, 6),
        "in offset by 4 bytes": (f32, x.view.view(-1)[1:], out.view, N, IH, IW, 4, 8, 8),
        "out offset by 4 bytes": (f32, x.view, out.view.view(-1)[1:], N, IH, IW, 4, 8, 8),
        "dtype 7": (7, x.view, out.view, N, IH, IW, 8, 8, 8),
        "2^30 pixel rows": (f32, x.view, out.view, 1, 16384, 16384, 8, 8, 8),
        "in null": (f32, None, out.view, N, IH, IW, 8, 8, 8),
        "out null": (f32, x.view, None, N, IH, IW, 8, 8, 8),
    }
    for what, args in refused.items():
        with pytest.raises(ValueError):
            lib.call("rbvae_nearest2x_rows", *args)
        torch.cuda.synchronize()
        assert torch.equal(bits(out.buf), bits(before)), what
    print(f"\nnearest2x_rows: {len(refused)} refused calls raised ValueError and wrote nothing")
