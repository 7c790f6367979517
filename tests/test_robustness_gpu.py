"""GPU: robustness evaluation on raw frames (robustness.py) against the reference's one-frame-at-a-time host loop
(embedding_matching.py:209-299): every frame prepared on the host with PIL + torch (ToTensor -> perturbation ->
ToPILImage -> load_img_for_sd / ImageTransforms), then the same encoders with the same draws.  The codes are
bit-identical, the consistencies equal, and the winners / Hamming distances those of np.unique and Counter."""
import random
from collections import Counter

import numpy as np
import pytest
import torch

import sfv_amd as sfv
from _frames_ref import add_gaussian_noise, add_occlusion, contrastive_host, sd_host, to_pil_array, to_tensor

pytestmark = pytest.mark.gpu
pytest.importorskip("PIL")

F, H, W, FLAGS, LD = 60, 200, 360, [20, 40], 16
TARGET, RES, BATCH = (256, 136), 64, 24
PERTS = [(None, {}), ("gaussian_noise", {"std": 0.1}), ("occlusion", {"coverage": 0.2})]


def _video():
    """three states of 20 frames: a different colour layout per state, drifting a little from frame to frame"""
    rng = np.random.default_rng(2)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty((F, H, W, 3), dtype=np.uint8)
    for f in range(F):
        s = sfv.assign_label(f, FLAGS)
        base = np.stack([(xx * (s + 1) + f) % 256, (yy * (3 - s) + 2 * f) % 256,
                         np.where((xx // 40 + yy // 40 + s) % 2 == 0, 200, 40)], -1)
        out[f] = np.clip(base + rng.integers(-6, 7, base.shape), 0, 255)
    return out


@pytest.fixture(scope="module")
def setup():
    torch.manual_seed(0)
    enc = sfv.LDMEncoder("f32").cuda()
    pm = sfv.Seq2SeqBinaryVAE(4, 4, LD, LD, variant="percep", input_hw=(16, 32), compute_dtype="f32").cuda().eval()
    cm = sfv.Seq2SeqBinaryVAE(3, 3, LD, LD, variant="contrastive", input_hw=(RES, RES), compute_dtype="f32").cuda().eval()
    a = _video()
    return enc, pm, cm, a, torch.from_numpy(a).cuda()


def _draws(perceptual, pert, seed):
    g = torch.Generator().manual_seed(seed)
    ph, pw = (H, W) if perceptual else (RES, RES)
    d = {"u": torch.rand(F, LD, generator=g), "eps": torch.randn(F, 4, 16, 32, generator=g) if perceptual else None,
         "noise": torch.randn(F, 3, ph, pw, generator=g) if pert == "gaussian_noise" else None, "boxes": None}
    if pert == "occlusion":
        r = random.Random(seed)
        s = int(np.sqrt(0.2 * ph * pw))
        d["boxes"] = [(bx, r.randint(0, ph - s), s) for bx in (r.randint(0, pw - s) for _ in range(F))]
    return d


def _host_inputs(a, perceptual, pert, params, d):
    """the reference's per-frame preparation (embedding_matching.py:236-262)"""
    xs = []
    for i in range(F):
        img = a[i] if perceptual else None
        t = None if perceptual else contrastive_host(a[i], RES)          # ImageTransforms
        if pert is not None:
            t = to_tensor(img) if t is None else t
            if pert == "gaussian_noise":
                t = add_gaussian_noise(t, d["noise"][i:i + 1], params["std"], 0.0)
            else:
                t = add_occlusion(t, d["boxes"][i])
            img = to_pil_array(t)                                           # ToPILImage
            t = None
        if perceptual:
            xs.append(sd_host(img, TARGET))
        else:
            xs.append((to_tensor(img) if t is None else t)[None])
    return torch.cat(xs)


def _host_codes(model, x, d, enc):
    """the same encoders, in the device pipeline's batches, on the host-prepared inputs"""
    out = []
    for s in range(0, F, BATCH):
        xb = x[s:s + BATCH].cuda()
        if enc is not None:
            xb = enc.encode(xb, eps=d["eps"][s:s + BATCH].cuda())
        out.append(model.encode(xb[:, None], temperature=0.2, hard=True, noise_ratio=0.1,
                                u=d["u"][s:s + BATCH].cuda())[:, 0])
    return torch.cat(out).cpu()


def _np_consistency(codes, labels, n):
    pct, counts = [], []
    for s in range(n):
        v = codes[labels == s]
        counts.append(len(v))
        uq, c = np.unique(v, axis=0, return_counts=True)
        pct.append(np.mean(np.all(v == uq[np.argmax(c)], axis=1)))
    return np.dot(pct, counts) / sum(counts), pct


@pytest.mark.parametrize("perceptual", [True, False], ids=["percep", "contrastive"])
@pytest.mark.parametrize("pert,params", PERTS, ids=["clean", "noise", "occlusion"])
def test_codes_match_host_loop(setup, perceptual, pert, params):
    enc, pm, cm, a, frames = setup
    model = pm if perceptual else cm
    d = _draws(perceptual, pert, 17)
    kw = dict(ldm_encoder=enc if perceptual else None, temperature=0.2, noise_ratio=0.1, batch=BATCH, u=d["u"],
              noise=d["noise"], boxes=d["boxes"], eps=d["eps"], target=TARGET, resolution=RES)
    idx = list(range(F))
    codes, labels = sfv.state_codes_under(model, frames, idx, FLAGS, pert, params, **kw)
    ref = _host_codes(model, _host_inputs(a, perceptual, pert, params, d), d, enc if perceptual else None)
    assert torch.equal(codes.cpu(), ref)
    assert list(labels) == [sfv.assign_label(i, FLAGS) for i in idx]
    avg, pct = sfv.state_consistency_under(model, frames, idx, FLAGS, pert, params, **kw)
    ravg, rpct = _np_consistency(ref.numpy(), labels, 3)
    assert abs(avg - ravg) <= 1e-12 and np.allclose(pct, rpct, rtol=0, atol=1e-12)
    if pert == "occlusion":            # the default boxes are the reference's `random` draws
        random.seed(23)
        c1, _ = sfv.state_codes_under(model, frames, idx, FLAGS, pert, params, **dict(kw, boxes=None))
        random.seed(23)
        ph, pw = (H, W) if perceptual else (RES, RES)
        s = int(np.sqrt(0.2 * ph * pw))
        boxes = []
        for _ in range(F):
            bx = random.randint(0, pw - s)
            boxes.append((bx, random.randint(0, ph - s), s))
        c2, _ = sfv.state_codes_under(model, frames, idx, FLAGS, pert, params, **dict(kw, boxes=boxes))
        assert torch.equal(c1, c2)


def _counter_winner(v):
    return np.array(Counter([tuple(r) for r in v]).most_common(1)[0][0])


def test_most_common_and_hamming(setup):
    enc, pm, cm, a, frames = setup
    d = _draws(False, None, 5)
    codes, labels = sfv.state_codes_under(cm, frames, list(range(F)), FLAGS, u=d["u"], batch=BATCH, resolution=RES)
    # model codes, and crafted codes with tied counts (where the two tie rules disagree)
    rng = np.random.default_rng(1)
    pool = rng.integers(0, 2, (6, LD))
    crafted = np.concatenate([pool[[3, 1, 3, 1, 0] * 4], pool[[5, 2, 2, 5, 4] * 4], pool[[0, 1, 2, 3, 4] * 4]])
    for c in (codes, torch.from_numpy(crafted).float().cuda()):
        host = c.cpu().numpy().astype(np.int64)
        lex, cnt = sfv.most_common_codes(c, labels, 3, tie="lexicographic")
        first, _ = sfv.most_common_codes(c, labels, 3, tie="first")
        for s in range(3):
            v = host[labels == s]
            uq, n = np.unique(v, axis=0, return_counts=True)
            assert np.array_equal(lex[s], uq[np.argmax(n)]) and cnt[s] == n.max()
            assert np.array_equal(first[s], _counter_winner(v))
        dist, mean = sfv.adjacent_hamming(first)
        ref = [int(np.sum(first[i] != first[i + 1])) for i in range(2)]
        assert list(dist) == ref and mean == np.mean(ref)
    assert not np.array_equal(sfv.most_common_codes(torch.from_numpy(crafted).float().cuda(), labels, 3)[0],
                              sfv.most_common_codes(torch.from_numpy(crafted).float().cuda(), labels, 3, "first")[0])


def test_reference_draws_order():
    """per frame: randn_like [1,3,H,W], randn [1,4,h,w], rand [1,L], from the global CPU generator"""
    torch.manual_seed(4)
    d = sfv.reference_draws(3, LD, noise_hw=(5, 6), latent_hw=(2, 3))
    torch.manual_seed(4)
    for i in range(3):
        assert torch.equal(d["noise"][i:i + 1], torch.randn(1, 3, 5, 6))
        assert torch.equal(d["eps"][i:i + 1], torch.randn(1, 4, 2, 3))
        assert torch.equal(d["u"][i:i + 1], torch.rand(1, LD))
