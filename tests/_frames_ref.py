"""Host restatements of the reference's frame preprocessing (Pillow + numpy + torch CPU), shared by the frame and
robustness tests: the yardstick csrc/frames.hip is held to."""
import numpy as np
import torch

CASES = [  # (in W, in H, out W, out H, filter): down- and upscale, one axis only, odd sizes, both reference filters
    (131, 83, 64, 40, "lanczos"), (70, 50, 33, 123, "lanczos"), (61, 37, 61, 20, "lanczos"),
    (45, 32, 98, 32, "lanczos"), (640, 360, 256, 256, "bilinear"), (97, 61, 256, 256, "bilinear"),
    (33, 17, 200, 9, "bilinear"), (255, 143, 64, 64, "bilinear"), (1280, 720, 1280, 704, "lanczos"),
]


def pil_filter(name):
    from PIL import Image
    return {"lanczos": Image.LANCZOS, "bilinear": Image.BILINEAR}[name]


def pil_resize(a, size, filt):
    """Image.resize of one u8 [H,W,3] array."""
    from PIL import Image
    return np.asarray(Image.fromarray(a).resize(tuple(size), pil_filter(filt)))


def frame_image(rng, w, h, n=None):
    """u8 frames with every byte value, smooth ramps and sharp edges (the filters' negative lobes clip)."""
    shape = (h, w, 3) if n is None else (n, h, w, 3)
    a = rng.integers(0, 256, shape, dtype=np.int64)
    ramp = (np.arange(w)[None, :, None] * 7 + np.arange(h)[:, None, None] * 3) % 256
    a = np.where(rng.random(shape) < 0.5, a, ramp)
    return a.astype(np.uint8)


def to_tensor(a):
    """T.ToTensor of an RGB PIL image / u8 [H,W,3] array: permute, float, div(255)."""
    return torch.from_numpy(np.array(a, copy=True)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def to_pil_array(t):
    """T.ToPILImage of a [3,H,W] f32 tensor, as the array Image.fromarray receives: mul(255).byte(), HWC."""
    return np.transpose(t.mul(255).byte().numpy(), (1, 2, 0))


def add_gaussian_noise(t, noise, std=0.1, mean=0.0):
    """embedding_matching.py:141-158 with the randn_like draw given."""
    t = t.unsqueeze(0) if t.dim() == 3 else t
    return torch.clamp(t + (noise.reshape(t.shape) * std + mean), 0, 1).squeeze()


def add_occlusion(t, box):
    """embedding_matching.py:163-193 with the square's (x, y, size) given."""
    t = t.unsqueeze(0) if t.dim() == 3 else t
    x, y, s = (int(v) for v in box)
    o = t.clone()
    o[:, :, y:y + s, x:x + s] = 0.5
    return o.squeeze()


def sd_host(a, target=(1280, 720)):
    """load_img_for_sd (embedding_matching.py:318-338) of one u8 [H,W,3] array -> f32 [1,3,h,w]."""
    from PIL import Image
    im = Image.fromarray(a).resize(tuple(target), Image.LANCZOS)
    w, h = (v - v % 32 for v in target)
    if (w, h) != tuple(target):
        im = im.resize((w, h), Image.LANCZOS)
    x = np.array(im).astype(np.float32) / 255.0
    x = torch.from_numpy(x[None].transpose(0, 3, 1, 2))
    return 2. * x - 1.


def contrastive_host(a, resolution=256):
    """ImageTransforms (contrastive_RBVAE_train.py:110-114): T.Resize((r, r)) on a PIL image = BILINEAR, ToTensor."""
    return to_tensor(pil_resize(a, (resolution, resolution), "bilinear"))
