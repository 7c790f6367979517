"""Write tests/golden/frames_resample.npz: seeded u8 frames and their PIL.Image.resize outputs, so the GPU test of
the resampler (tests/test_frames_gpu.py) has a Pillow yardstick that needs no Pillow where it runs.

    python tools/make_frames_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _frames_ref import frame_image, pil_resize  # noqa: E402

# (in W, in H, out W, out H, filter, frames): small versions of the reference's chains plus odd, one-axis and upscales
CASES = [(96, 54, 64, 36, "lanczos", 2), (64, 36, 64, 32, "lanczos", 1), (61, 37, 29, 20, "lanczos", 1),
         (35, 25, 17, 62, "lanczos", 1), (47, 31, 24, 24, "bilinear", 1), (20, 15, 45, 35, "bilinear", 1),
         (40, 30, 31, 30, "bilinear", 1)]


def main():
    rng = np.random.default_rng(20261016)
    out = {}
    for i, (iw, ih, ow, oh, filt, n) in enumerate(CASES):
        a = frame_image(rng, iw, ih, n)
        out[f"case{i}/meta"] = np.array([iw, ih, ow, oh, n], dtype=np.int32)
        out[f"case{i}/filter"] = np.array(filt)
        out[f"case{i}/input"] = a
        out[f"case{i}/output"] = np.stack([pil_resize(x, (ow, oh), filt) for x in a])
    path = os.path.join(ROOT, "tests", "golden", "frames_resample.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
