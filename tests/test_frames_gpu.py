"""GPU: the raw-frame front end (csrc/frames.hip through frames.py) against the reference's host preprocessing --
Pillow's resize byte for byte, ToTensor -> perturbation -> ToPILImage byte for byte, and the f32 model inputs of
load_img_for_sd / ImageTransforms bit for bit."""
import os

import numpy as np
import pytest
import torch

import sfv_amd as sfv
from _frames_cases import _boundary_noise
from _frames_ref import (CASES, add_gaussian_noise, add_occlusion, contrastive_host, frame_image, pil_resize, sd_host,
                         to_pil_array, to_tensor)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames_resample.npz")


def test_resize_matches_golden():
    """Pillow's outputs recorded in tests/golden (no Pillow needed here)."""
    g = np.load(GOLDEN, allow_pickle=False)
    n_cases = len({k.split("/")[0] for k in g.files})
    assert n_cases >= 7
    for i in range(n_cases):
        iw, ih, ow, oh, n = (int(v) for v in g[f"case{i}/meta"])
        x = torch.from_numpy(g[f"case{i}/input"]).cuda()
        got = sfv.resize_u8(x, (ow, oh), str(g[f"case{i}/filter"])).cpu().numpy()
        assert got.shape == (n, oh, ow, 3)
        assert np.array_equal(got, g[f"case{i}/output"]), (i, iw, ih, ow, oh)


@pytest.mark.parametrize("iw,ih,ow,oh,filt", CASES)
def test_resize_matches_pillow(iw, ih, ow, oh, filt):
    pytest.importorskip("PIL")
    a = frame_image(np.random.default_rng(iw * 7 + ih), iw, ih, 3)
    x = torch.from_numpy(a).cuda()
    got = sfv.resize_u8(x, (ow, oh), filt).cpu().numpy()
    for j in range(3):
        assert np.array_equal(got[j], pil_resize(a[j], (ow, oh), filt)), j
    # an unaligned batch view (rows of 3 * odd bytes start anywhere): the same bytes
    if (iw * ih) % 2:
        sub = x[1:]
        assert sub.data_ptr() % 4 != 0
        assert np.array_equal(sfv.resize_u8(sub, (ow, oh), filt).cpu().numpy(), got[1:])


def test_reference_chain_and_copy():
    """1920 x 1080 -> 1280 x 720 -> 1280 x 704 (load_img), a batch of 2; the same size is a copy."""
    pytest.importorskip("PIL")
    a = frame_image(np.random.default_rng(11), 1920, 1080, 2)
    x = torch.from_numpy(a).cuda()
    mid = sfv.resize_u8(x, (1280, 720), "lanczos")
    fin = sfv.resize_u8(mid, (1280, 704), "lanczos").cpu().numpy()
    mid = mid.cpu().numpy()
    for j in range(2):
        m = pil_resize(a[j], (1280, 720), "lanczos")
        assert np.array_equal(mid[j], m)
        assert np.array_equal(fin[j], pil_resize(m, (1280, 704), "lanczos"))
    same = sfv.resize_u8(x, (1920, 1080), "bilinear")
    assert same.data_ptr() != x.data_ptr() and torch.equal(same, x)


def test_perturb_matches_torch():
    rng = np.random.default_rng(3)
    H, W = 37, 53
    a = frame_image(rng, W, H, 4)
    x = torch.from_numpy(a).cuda()
    std, mean = 0.1, 0.0
    noise = torch.randn(4, 3, H, W, generator=torch.Generator().manual_seed(5))
    noise[:2] = torch.stack([_boundary_noise(a[j], std, rng) for j in range(2)])
    got = sfv.perturb_u8(x, "gaussian_noise", std=std, mean=mean, noise=noise.cuda()).cpu().numpy()
    for j in range(4):
        ref = to_pil_array(add_gaussian_noise(to_tensor(a[j]), noise[j:j + 1], std, mean))
        assert np.array_equal(got[j], ref), j
    got = sfv.perturb_u8(x, "gaussian_noise", std=0.3, mean=0.05, noise=noise.cuda()).cpu().numpy()
    for j in range(4):
        assert np.array_equal(got[j], to_pil_array(add_gaussian_noise(to_tensor(a[j]), noise[j:j + 1], 0.3, 0.05)))
    boxes = [(0, 0, 10), (40, 20, 17), (5, 30, 7), (52, 36, 1)]
    got = sfv.perturb_u8(x, "occlusion", boxes=boxes).cpu().numpy()
    for j in range(4):
        assert np.array_equal(got[j], to_pil_array(add_occlusion(to_tensor(a[j]), boxes[j]))), j
    assert got[0, 0, 0, 0] == 127                                   # 0.5 * 255 truncated
    # the default boxes are add_occlusion's `random` draws, in frame order
    import random
    random.seed(9)
    d = sfv.perturb_u8(x, "occlusion", coverage=0.2).cpu().numpy()
    random.seed(9)
    s = int(np.sqrt(0.2 * H * W))
    ref_boxes = []
    for _ in range(4):
        bx = random.randint(0, W - s)
        ref_boxes.append((bx, random.randint(0, H - s), s))
    assert np.array_equal(d, sfv.perturb_u8(x, "occlusion", boxes=ref_boxes).cpu().numpy())
    # the default noise is a device draw from the generator: reproducible
    g1, g2 = torch.Generator("cuda").manual_seed(1), torch.Generator("cuda").manual_seed(1)
    assert torch.equal(sfv.perturb_u8(x, "gaussian_noise", generator=g1), sfv.perturb_u8(x, "gaussian_noise", generator=g2))


def test_model_inputs_match_host_pipeline():
    pytest.importorskip("PIL")
    rng = np.random.default_rng(4)
    a = frame_image(rng, 360, 200, 3)
    x = torch.from_numpy(a).cuda()
    got = sfv.sd_input(x, target=(256, 136))
    assert got.shape == (3, 3, 128, 256) and got.dtype == torch.float32
    ref = torch.cat([sd_host(a[j], (256, 136)) for j in range(3)])
    assert torch.equal(got.cpu(), ref)
    buf = torch.full((3 * 3 * 128 * 256,), float("nan"), device="cuda")
    sfv.sd_input(x, target=(256, 136), out=buf)
    assert torch.equal(buf.view(3, 3, 128, 256).cpu(), ref)
    got = sfv.contrastive_input(x, resolution=64)
    ref = torch.stack([contrastive_host(a[j], 64) for j in range(3)])
    assert got.shape == (3, 3, 64, 64) and torch.equal(got.cpu(), ref)
    # the default SD target: 1280 x 720 then 1280 x 704
    b = frame_image(rng, 480, 270, 1)
    assert torch.equal(sfv.sd_input(torch.from_numpy(b).cuda()).cpu(), sd_host(b[0]))


def test_bad_inputs_raise():
    x = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device="cuda")
    for bad in (x.float(), torch.zeros(2, 8, 8, 4, dtype=torch.uint8, device="cuda"), x.permute(0, 2, 1, 3),
                x[:, :, :, :3].expand(2, 8, 8, 3).transpose(1, 2), torch.zeros(8, 8, 3, dtype=torch.uint8, device="cuda")):
        with pytest.raises(ValueError):
            sfv.resize_u8(bad, (4, 4), "lanczos")
        with pytest.raises(ValueError):
            sfv.perturb_u8(bad, "occlusion", boxes=[(0, 0, 1)] * 2)
        with pytest.raises(ValueError):
            sfv.u8_to_input(bad)
    with pytest.raises(ValueError):
        sfv.resize_u8(x, (4, 4), "bicubic")
    with pytest.raises(ValueError):
        sfv.perturb_u8(x, "blur")
    with pytest.raises(ValueError):
        sfv.perturb_u8(x, "gaussian_noise", noise=torch.zeros(2, 3, 8, 7, device="cuda"))
    with pytest.raises(ValueError):
        sfv.sd_input(x, out=torch.zeros(5, device="cuda"))


def test_extract_embeddings_matches_encode():
    """extract_embeddings = sd_input + LDMEncoder.encode per chunk, rows in frame order; to_reference_dict keys."""
    torch.manual_seed(0)
    enc = sfv.LDMEncoder("f32").cuda()
    a = frame_image(np.random.default_rng(8), 100, 60, 5)
    x = torch.from_numpy(a).cuda()
    eps = torch.randn(5, 4, 8, 16)
    tab = sfv.extract_embeddings(enc, x, None, chunk=2, eps=eps, target=(128, 72))
    assert tab.shape == (5, 4, 8, 16)
    for s in (0, 2, 4):
        ref = enc.encode(sfv.sd_input(x[s:s + 2], (128, 72)), eps=eps[s:s + 2].cuda())
        assert torch.equal(tab[s:s + 2], ref)
    d = sfv.to_reference_dict(tab, [10, 11, 12, 13, 14])
    assert sorted(d) == [f"{i:010d}.jpg" for i in range(10, 15)] and d["0000000012.jpg"].shape == (1, 4, 8, 16)
    ds = sfv.DeviceStatePairDataset(tab, [(0, 3), (3, 5)], test_pct=0.0, val_pct=0.0)
    assert torch.equal(ds.frames([4]), tab[4:5])
