"""Latent extraction from raw u8 frames: sd_input (two LANCZOS resizes + 2x/255-1 on the device) and the LDM encode,
frames/s and the time split between them (get_percep_embeddings.py's loop as batched device work).

    python tools/run_extract.py [--size 1920x1080] [--chunk 16] [--chunks 4] [--dtype bf16]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import sfv_amd as sfv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080", help="source frame W x H")
    ap.add_argument("--target", default="1280x720", help="load_img's resize target W x H (then rounded down to /32)")
    ap.add_argument("--chunk", type=int, default=16, help="frames per sd_input + encode")
    ap.add_argument("--chunks", type=int, default=4, help="timed chunks")
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "f32"))
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split("x"))
    target = tuple(int(v) for v in a.target.split("x"))
    torch.manual_seed(0)
    enc = sfv.LDMEncoder(a.dtype).cuda()
    g = torch.Generator("cuda").manual_seed(1)
    frames = torch.randint(0, 256, (a.chunk, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    w, h = sfv.pkg.frames.sd_target(target)
    x = torch.empty(a.chunk, 3, h, w, device="cuda")
    lat = torch.empty(a.chunk, 4, h // 8, w // 8, device="cuda")
    for _ in range(2):                                   # warm-up: coefficient tables, packed weights
        sfv.sd_input(frames, target, out=x)
        enc.encode(x, sample=False, out=lat)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t_pre = t_enc = 0.0
    t0 = time.perf_counter()
    for _ in range(a.chunks):
        ev[0].record()
        sfv.sd_input(frames, target, out=x)
        ev[1].record()
        enc.encode(x, sample=False, out=lat)
        ev[2].record()
        ev[2].synchronize()
        t_pre += ev[0].elapsed_time(ev[1])
        t_enc += ev[1].elapsed_time(ev[2])
    wall = time.perf_counter() - t0
    n = a.chunk * a.chunks
    print(f"{W}x{H} -> {w}x{h} ({a.dtype}), {n} frames in chunks of {a.chunk}: {n / wall:.1f} frames/s; "
          f"per frame sd_input {t_pre / n:.3f} ms ({100 * t_pre / (t_pre + t_enc):.1f} %), "
          f"encode {t_enc / n:.3f} ms; latent {tuple(lat.shape[1:])}", flush=True)


if __name__ == "__main__":
    main()
