"""The LDM decoder's reference material without a GPU: the CPU restatement (tests/_ldm_decoder_ref.py) against outputs of the
reference's own Decoder class (tests/golden/ldm_decoder.npz, tools/make_ldm_decoder_golden.py), the parity fold of Upsample
against interpolate + conv2d in float64, interpolate_embeddings against the reference script's arrays, and the ABI.

e32 = max |float32 restatement - float64 restatement| over both fixture outputs = 3.04e-6 (case a 2.83e-6, case b 3.04e-6):
the rounding floor of ONE float32 evaluation of the decoder.  tests/test_ldm_decoder_gpu.py gates the device's float32
decoder at 8 e32; test_e32_is_what_the_gpu_gate_assumes pins the figure."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _ldm_decoder_ref as DR
from _golden import load

E32 = 3.04e-6          # measured, see the module docstring; the GPU test's gate is 8 * E32


@pytest.fixture(scope="module")
def fixture():
    g = load("ldm_decoder")
    return g, DR.init_params(int(g["meta/seed"]))


def test_init_params_match_fixture_order_and_paramsums(fixture):
    g, p = fixture
    assert list(p.keys()) == [str(k) for k in g["meta/keys"]]
    assert len(p) == 140 and sum(v.numel() for v in p.values()) == 49_490_199
    for k, v in p.items():
        cs = g[f"paramsum/{k}"]
        assert abs(float(v.double().sum()) - cs[0]) <= 1e-9 * max(1.0, cs[1]), k
        assert abs(float(v.double().abs().sum()) - cs[1]) <= 1e-9 * cs[1], k


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_reproduces_reference_decoder(fixture, tag):
    g, p = fixture
    with torch.no_grad():
        out = DR.decode(p, torch.from_numpy(g[f"z_{tag}"]))
    assert out.shape == g[f"out_{tag}"].shape
    np.testing.assert_allclose(out.numpy(), g[f"out_{tag}"], atol=5e-6)          # test_oracle_golden.py's standard


def test_e32_is_what_the_gpu_gate_assumes(fixture):
    g, p = fixture
    e32 = 0.0
    with torch.no_grad():
        for tag in "ab":
            z = torch.from_numpy(g[f"z_{tag}"])
            e32 = max(e32, float((DR.decode(p, z).double() - DR.decode(p, z.double())).abs().max()))
    print(f"e32 = {e32:.4g}")
    assert 0.5 * E32 <= e32 <= 2 * E32, e32         # the figure moves a little with the host's convolution library


@pytest.mark.parametrize("h,w", [(1, 1), (7, 6), (16, 17)])
@pytest.mark.parametrize("Ci", [5, 64])
def test_fold_equals_interpolate_conv_f64(h, w, Ci):
    g = torch.Generator().manual_seed(100 * h + w + Ci)
    x = torch.randn(2, Ci, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(8, Ci, 3, 3, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), wt, padding=1)
    wf = DR.fold_upconv(wt, Kc=Ci + 3)
    assert bool((wf[:, :, Ci:] == 0).all())
    import sfv_amd as sfv
    # the folded weights through the PRODUCT's class descriptor (what LDMDecoder hands rbvae_gather_gemm, and the tap order
    # rbvae_upconv3x3_halo walks), and through the restated four-class form the GPU tests take their references from
    for got in (DR.gather_classes(x, wf, sfv.ldm.upconv_class_desc()), DR.upconv_folded(x, wf)):
        rel = float((got - ref).abs().max() / ref.abs().max())
        print(f"{h}x{w} Ci={Ci}: {rel:.3g}")
        assert rel <= 1e-12
    if h > 1:                                        # every named defect of the GPU test is far outside that
        for d in ("dropped_tap", "swapped_classes", "wrong_edge"):
            assert float((DR.upconv_folded(x, wf, d) - ref).abs().max() / ref.abs().max()) > 0.1, d
        bad = DR.upconv_folded(x, DR.fold_upconv(wt, defect="unfolded_w1"))
        assert float((bad - ref).abs().max() / ref.abs().max()) > 0.1


def test_class_descriptor_matches_product():
    import sfv_amd as sfv
    assert list(sfv.ldm.upconv_class_desc()) == DR.upconv_class_desc()


def test_interpolate_embeddings_bit_exact(fixture):
    import sfv_amd as sfv
    g, _ = fixture
    z0, z1 = torch.from_numpy(g["interp/z0"]), torch.from_numpy(g["interp/z1"])
    for method in ("linear", "spherical"):
        got = sfv.interpolate_embeddings(z0, z1, steps=5, method=method)
        assert len(got) == 5 and all(t.dtype == torch.float32 for t in got)
        assert np.array_equal(torch.stack(got).numpy(), g[f"interp/{method}"]), method
    same = sfv.interpolate_embeddings(z0, z0.clone(), steps=5, method="spherical")
    assert np.array_equal(torch.stack(same).numpy(), g["interp/same_spherical"])
    with pytest.raises(ValueError):
        sfv.interpolate_embeddings(z0, z1, method="cubic")


def test_identical_inputs_take_the_lerp_branch():
    """|z| = 8 and z / 8 exactly representable: dot = 1, omega = 0, sin(omega) = 0 -- the slerp weights would be 0 / 0."""
    import sfv_amd as sfv
    g = torch.Generator().manual_seed(3)
    z = 0.5 * (2.0 * torch.randint(0, 2, (4, 8, 8), generator=g).float() - 1.0)
    got = torch.stack(sfv.interpolate_embeddings(z, z.clone(), steps=5, method="spherical"))
    assert not bool(torch.isnan(got).any())
    want = torch.stack([(1.0 - i / 4) * z + (i / 4) * z for i in range(5)])
    assert torch.equal(got, want)


NEW_ENTRY_POINTS = ["rbvae_upconv_fold", "rbvae_upconv3x3_halo_ok", "rbvae_upconv3x3_halo", "rbvae_nearest2x_rows",
                    "rbvae_latent_rows", "rbvae_decoded_to_image"]


def test_header_declares_and_library_exports_the_decoder_entry_points():
    import sfv_amd as sfv
    protos = sfv._lib.parse_header()
    for n in NEW_ENTRY_POINTS:
        assert n in protos, n
    assert [nm for _, nm in protos["rbvae_upconv3x3_halo"][1]][-3:] == ["lda", "ldo", "stream"]
    assert os.path.exists(sfv._lib.LIB_PATH), "build the library first"
    lib = ctypes.CDLL(sfv._lib.LIB_PATH)
    for n in NEW_ENTRY_POINTS:
        assert hasattr(lib, n), n
    # the shape query is host code: it answers without a GPU
    ok = lib.rbvae_upconv3x3_halo_ok
    assert ok(1, 1, 5, 5, 64, 128) == 1 and ok(0, 1, 5, 5, 32, 128) == 1
    assert ok(1, 1, 4, 12, 64, 128) == 0 and ok(1, 1, 12, 4, 64, 128) == 0
    assert ok(1, 1, 8, 8, 32, 128) == 0 and ok(1, 1, 8, 8, 64, 64) == 0 and ok(2, 1, 8, 8, 64, 128) == 0


def test_decoder_module_keys_and_errors_without_a_gpu(fixture):
    import sfv_amd as sfv
    g, p = fixture
    torch.manual_seed(int(g["meta/seed"]))
    m = sfv.LDMDecoder(compute_dtype="f32")
    sd = m.state_dict()
    assert list(sd.keys()) == list(p.keys())
    for k in p:
        assert torch.equal(sd[k], p[k]), k
    with pytest.raises(RuntimeError):
        m.decode(torch.zeros(1, 4, 8, 8))
    with pytest.raises(ValueError):
        sfv.LDMDecoder(upsample_impl="bilinear")
