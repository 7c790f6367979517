"""Frozen LDM VAE decode: latents -> u8 frames (frames/s), the counterpart of run_ldm.py.

  python tools/run_ldm_decode.py [NxS ...]            frames/s of LDMDecoder.decode_u8 for N frames of S x S (default 8x256 4x512)
  python tools/run_ldm_decode.py --upsample           the three Upsample forms alone (HIP events, forms alternating) at the
                                                      shapes of 512 x 512 frames, N = 4: 64^2 -> 128^2 and 128^2 -> 256^2 at
                                                      512 channels, 256^2 -> 512^2 at 256 channels
  python tools/run_ldm_decode.py --interpolate A.png B.png [--outdir DIR] [--steps 5] [--method linear|spherical] [--ckpt F]
                                                      encode -> interpolate -> decode -> PNG
                                                      (scripts/pretrained_model_experiments/ldm_embedding_interpol.py)
LDM_DTYPE=f32|bf16 (default bf16), LDM_UPSAMPLE=halo|gather|unfolded (default halo), LDM_ITERS (default 5),
LDM_HALO_ALL=1: "halo" runs the folded kernel on every shape it covers instead of the shapes the dispatch rule names."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import sfv_amd as sfv  # noqa: E402

DTYPE = os.environ.get("LDM_DTYPE", "bf16")
ITERS = int(os.environ.get("LDM_ITERS", "5"))


def frames_per_s(shapes):
    torch.manual_seed(0)
    m = sfv.LDMDecoder(compute_dtype=DTYPE, upsample_impl=os.environ.get("LDM_UPSAMPLE", "halo"),
                       halo_where_covered=bool(int(os.environ.get("LDM_HALO_ALL", "0")))).cuda()
    for N, S in shapes:
        z = torch.randn(N, 4, S // 8, S // 8, device="cuda") * 0.18215 * 4
        for _ in range(2):
            m.decode_u8(z)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(ITERS):
            out = m.decode_u8(z)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / ITERS
        print(f"{S}x{S}: {N / dt:.1f} frames/s, {dt * 1e3:.1f} ms per {N} frames, {m.upsample_impl} {m.upsample_dispatch}, "
              f"frames {tuple(out.shape)}", flush=True)


def upsample_forms(N=4, rounds=7):
    """Each Upsample of a 512 x 512 decode alone, per form: median of `rounds` HIP-event timings, the forms taking turns."""
    torch.manual_seed(0)
    tdt = torch.float32 if DTYPE == "f32" else torch.bfloat16
    dec = {impl: sfv.LDMDecoder(compute_dtype=DTYPE, upsample_impl=impl, halo_where_covered=True)
           for impl in ("halo", "gather", "unfolded")}
    sd = dec["halo"].state_dict()
    for impl, m in dec.items():
        m.load_state_dict(sd)
        m.cuda()
        m._check_input(torch.zeros(1, 4, 8, 8, device="cuda"))                  # packs the weights
    for lvl, H, C in ((3, 64, 512), (2, 128, 512), (1, 256, 256)):
        x = torch.randn(N * H * H, C, device="cuda").to(tdt)
        times = {impl: [] for impl in dec}
        for r in range(rounds + 1):
            for impl, m in dec.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                m._upsample(f"decoder.up.{lvl}.upsample.conv", x, N, H, H, C)
                e1.record()
                e1.synchronize()
                if r:
                    times[impl].append(e0.elapsed_time(e1) * 1e3)
        flop = 2.0 * N * 4 * H * H * C * C * 9
        line = ", ".join(f"{impl} {sorted(t)[len(t) // 2]:.0f} us (min {min(t):.0f})" for impl, t in times.items())
        best = min(times, key=lambda k: sorted(times[k])[len(times[k]) // 2])
        print(f"upsample {H}^2 -> {2 * H}^2, {C} channels, N = {N}, {DTYPE}: {line}; fastest {best}; as written "
              f"{flop / 1e9:.0f} GFLOP, folded {flop * 4 / 9 / 1e9:.0f}", flush=True)


def interpolate(a, b, outdir, steps, method, ckpt):
    import numpy as np
    from PIL import Image
    enc, dec = sfv.LDMEncoder(compute_dtype=DTYPE), sfv.LDMDecoder(compute_dtype=DTYPE)
    if ckpt:
        sd = torch.load(ckpt, map_location="cpu")
        sd = sd.get("state_dict", sd)
        enc.load_state_dict(sd)
        dec.load_state_dict(sd)
    enc, dec = enc.cuda(), dec.cuda()
    lat = []
    for path in (a, b):
        with Image.open(path) as im:                                      # load_img: sides rounded down to a multiple of 32
            u8 = torch.from_numpy(np.asarray(im.convert("RGB"))).cuda()[None]
        h, w = u8.shape[1] - u8.shape[1] % 32, u8.shape[2] - u8.shape[2] % 32
        x = sfv.u8_to_input(sfv.resize_u8(u8, (w, h), "lanczos"), "sd")
        lat.append(enc.encode(x)[0])
    zs = torch.stack(sfv.interpolate_embeddings(lat[0], lat[1], steps=steps, method=method)).cuda()
    frames = dec.decode_u8(zs, chunk=1).cpu().numpy()
    os.makedirs(outdir, exist_ok=True)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(os.path.join(outdir, f"interpolated_{i:05}.png"))
    print(f"{steps} frames {frames.shape[1:]} -> {outdir}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("shapes", nargs="*", help="NxS")
    ap.add_argument("--upsample", action="store_true")
    ap.add_argument("--interpolate", nargs=2, metavar=("IMG0", "IMG1"))
    ap.add_argument("--outdir", default="outputs/interpolation")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--method", default="linear", choices=["linear", "spherical"])
    ap.add_argument("--ckpt", default=None)
    o = ap.parse_args()
    if o.upsample:
        upsample_forms()
    elif o.interpolate:
        interpolate(o.interpolate[0], o.interpolate[1], o.outdir, o.steps, o.method, o.ckpt)
    else:
        frames_per_s([(int(s.split("x")[0]), int(s.split("x")[1])) for s in o.shapes] or [(8, 256), (4, 512)])
