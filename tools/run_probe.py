"""Linear probe evaluation (linear_regression_eval.py:97-151) on a frames folder or on synthetic frames: the metrics, the
device time of each pass, the bytes each pass moves and its HBM floor, and -- where scikit-learn imports and the f32
arrays fit the host limit -- the host time of the reference's own calls (f32) on the same arrays.

    python tools/run_probe.py [--frames 128] [--res 256] [--latent 32] [--embedding h|z|random]
                              [--frames-dir DIR --first 0] [--src 480x270] [--host-limit-gb 2] [--repeat 3]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sfv_amd as sfv  # noqa: E402

HBM_BPS = 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128, help="number of frames (the script: 128)")
    ap.add_argument("--res", type=int, default=256, help="ImageTransforms' resolution")
    ap.add_argument("--latent", type=int, default=32)
    ap.add_argument("--embedding", default="h", choices=("h", "z", "random"),
                    help="h / z: a freshly initialised contrastive model; random: f32 normal embeddings, no model")
    ap.add_argument("--frames-dir", default=None, help="folder of %%010d.jpg frames (default: synthetic u8 frames)")
    ap.add_argument("--first", type=int, default=0, help="first frame number of --frames-dir")
    ap.add_argument("--src", default="480x270", help="synthetic source frame W x H")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--host-limit-gb", type=float, default=2.0, help="largest f32 target array handed to scikit-learn")
    ap.add_argument("--repeat", type=int, default=3, help="timed runs of the probe (the fastest is reported)")
    a = ap.parse_args()
    F, r, Ld = a.frames, a.res, a.latent
    torch.manual_seed(0)
    g = torch.Generator("cuda").manual_seed(1)
    chunk = 256
    if a.embedding == "random":
        # uniform random u8 frames at the probe's resolution, written chunk by chunk
        targets = torch.empty((F, r, r, 3), dtype=torch.uint8, device="cuda")
        for s in range(0, F, chunk):
            e = min(F, s + chunk)
            targets[s:e] = torch.randint(0, 256, (e - s, r, r, 3), dtype=torch.uint8, device="cuda", generator=g)
        emb = torch.randn((F, Ld), generator=torch.Generator().manual_seed(2))
    else:
        model = sfv.Seq2SeqBinaryVAE(3, 3, Ld, Ld, variant="contrastive", input_hw=(r, r)).cuda().eval()
        targets = torch.empty((F, r, r, 3), dtype=torch.uint8, device="cuda")
        emb = torch.empty((F, Ld), dtype=torch.float32, device="cuda")
        W, H = (int(v) for v in a.src.split("x"))
        t0 = time.perf_counter()
        for s in range(0, F, chunk):
            e = min(F, s + chunk)
            if a.frames_dir:
                src = sfv.load_frames(a.frames_dir, range(a.first + s, a.first + e))
            else:
                src = torch.randint(0, 256, (e - s, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
            emb[s:e], targets[s:e] = sfv.frame_embeddings(model, src, r, 0.5, a.embedding, a.batch)
        torch.cuda.synchronize()
        print(f"embedded {F} frames ({a.embedding}) in {time.perf_counter() - t0:.2f} s", flush=True)

    best = None
    for _ in range(max(1, a.repeat) + 1):                   # the first run warms up
        tm = {}
        res = sfv.linear_probe(emb, targets, timings=tm)
        if best is None or sum(tm.values()) < sum(best.values()):
            best = tm
    P, M, n, m = 3 * r * r, Ld + 1, res.n_train, res.n_test
    print(f"{F} frames, L = {Ld}, P = {P}: train {n}, test {m}, constant targets {res.n_constant_targets}")
    print(f"r2 {res.r2:.6f}  mse {res.mse:.6e}  mae {res.mae:.6e}  evs {res.evs:.6f}")
    slabs = sfv._lib.query("rbvae_probe_xty_slabs", n, M, P)
    mgroups = -(-(-(-M // 16)) // 3)
    moved = {
        "xty": n * P * mgroups + M * P * 8 * (1 if slabs == 1 else 2 * slabs + 1),
        "intercept": M * P * 8 + P + P * 8,
        "residual": m * P + M * P * 8 + 5 * P * 8,
        "finish": 5 * P * 8 + 2 * P * 8,
    }
    for k in ("xty", "intercept", "residual", "finish"):
        floor_ms = moved[k] / HBM_BPS * 1e3
        print(f"  {k:9s} {best[k]:9.3f} ms   {moved[k] / 1e6:10.1f} MB   HBM floor {floor_ms:8.3f} ms "
              f"({100 * floor_ms / best[k]:5.1f} % of the time)")
    mp, kp = -(-M // 16) * 16, -(-n // 16) * 16
    print(f"  xty: {slabs} K slab(s); f64 matrix-core rate {2.0 * mp * kp * P / (best['xty'] * 1e-3) / 1e12:.2f} TFLOP/s "
          f"(M padded to {mp}, {kp} rows)")
    print(f"  device total {sum(best.values()):.3f} ms")

    try:
        from sklearn.linear_model import LinearRegression
        from sklearn.metrics import explained_variance_score, mean_absolute_error, mean_squared_error, r2_score
        from sklearn.model_selection import train_test_split
    except ImportError:
        print("scikit-learn does not import here: no host timing")
        return
    if F * P * 4 > a.host_limit_gb * 2 ** 30:
        print(f"host reference skipped: the f32 targets are {F * P * 4 / 2 ** 30:.1f} GiB (--host-limit-gb {a.host_limit_gb})")
        return
    t0 = time.perf_counter()
    Yh = sfv.u8_to_input(targets, "totensor").reshape(F, -1).cpu().numpy()       # ToTensor + flatten, f32 [F, P]
    Xh = emb.float().cpu().numpy()
    t_copy = time.perf_counter() - t0
    t0 = time.perf_counter()
    Xtr, Xte, ytr, yte = train_test_split(Xh, Yh, test_size=0.2, random_state=42)
    model = LinearRegression()
    model.fit(Xtr, ytr)
    pred = model.predict(Xte)
    ref = (r2_score(yte, pred, multioutput="uniform_average"), mean_squared_error(yte, pred),
           mean_absolute_error(yte, pred), explained_variance_score(yte, pred, multioutput="uniform_average"))
    t_host = time.perf_counter() - t0
    print(f"scikit-learn f32 on the host ({os.environ.get('OMP_NUM_THREADS', '?')} threads): {t_host * 1e3:.1f} ms "
          f"(+ {t_copy * 1e3:.1f} ms to bring {Yh.nbytes / 1e6:.0f} MB of f32 targets to the host)")
    print(f"  r2 {ref[0]:.6f}  mse {ref[1]:.6e}  mae {ref[2]:.6e}  evs {ref[3]:.6f}")
    print(f"  device - host: r2 {res.r2 - ref[0]:.3g}  mse {res.mse - ref[1]:.3g}  mae {res.mae - ref[2]:.3g}  "
          f"evs {res.evs - ref[3]:.3g}")


if __name__ == "__main__":
    main()
