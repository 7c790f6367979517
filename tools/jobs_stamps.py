"""Rounds of the job launches inside the bench step: per-workgroup start / end stamps of run_jobs_k
(needs a library built with -DJOBS_STAMPS=1: tools/ab_variants.sh jobs.hip st:"-DJOBS_STAMPS=1", then
RBVAE_LIB=...librbvae_hip_st.so).  The bench's trainer (bench.py's shapes, set_data, one HIP graph per step) runs a few
steps; the stamps are those of the last replay, so every launch is read where it runs in the step, behind the
reductions and on cold data, not in a warm loop.  Per launch and per job kind: workgroups, first start, last end, median
life (us from the launch's first start) and the workgroups that started after the launch's first workgroup had ended
(a second round: they waited for a slot).
usage: python tools/jobs_stamps.py [--sized] [--map-order] [--steps 12]
  --sized        launch through rbvae_run_jobs_sized (fixed 36 992-byte tile, map order: the launch before rbvae_run_jobs_table)
  --map-order    rbvae_run_jobs_table without rbvae_job_launch_order's permutation"""
import argparse, os, random, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench as B
import sfv_amd as sfv
from importlib import import_module
trainer_mod = import_module("symbols-from-video_amd.trainer")
data_mod = import_module("symbols-from-video_amd.data")
J = import_module("symbols-from-video_amd.jobs")
L = sfv._lib
SLOTS, CAP = 16, 4096
KINDS = {0: "pack", 1: "permute+reduce", 2: "reduce rows", 3: "conv pack", 4: "conv reduce", 5: "gather", 6: "adam+pack", 7: "adam"}

ap = argparse.ArgumentParser()
ap.add_argument("--sized", action="store_true")
ap.add_argument("--map-order", action="store_true")
ap.add_argument("--steps", type=int, default=12)
a = ap.parse_args()
dev = torch.device("cuda", 0)

torch.manual_seed(1234)
model = sfv.Seq2SeqBinaryVAE(B.C_IN, B.C_IN, B.LATENT, B.LATENT, variant="percep", input_hw=B.HW, compute_dtype="bf16").to(dev).train()
g = torch.Generator(device="cpu").manual_seed(1234)
table = torch.randn(B.T_STATES * B.FRAMES_PER_STATE, B.C_IN, *B.HW, generator=g)
random.seed(1234)
segs = [(s * B.FRAMES_PER_STATE, (s + 1) * B.FRAMES_PER_STATE) for s in range(B.T_STATES)]
ds = data_mod.DeviceStatePairDataset(table, segs, mode="train", device=dev)
plan = ds.plan(torch.randperm(len(ds), generator=g), B.B_ITEMS)
tr = trainer_mod.FusedTrainer(model, lr=1e-3, alpha=B.ALPHA, beta_kl=B.BETA, bernoulli_p=B.BERN_P, noise_ratio=B.NOISE_R,
                              device_noise=True, use_graph=True, seed=1234)
tr.set_data(ds.table, plan)
eng = model._engine_for(tr.input_buffer(B.B_ITEMS, B.T_STATES, B.C_IN, *B.HW))
eng.table_launch = not a.sized
if a.sized or a.map_order:
    eng.jobs_heavy_first = 0

st = torch.zeros(SLOTS * CAP * 4, dtype=torch.int64, device=dev)
L.dbg_call("rbvae_dbg_jobs_stamps", st)            # before the capture: a captured launch keeps its slot
for _ in range(a.steps):
    tr.step(None, B.TAU)
torch.cuda.synchronize()
st.zero_()                                          # the eager warm-up launches' slots
tr.step(None, B.TAU)
torch.cuda.synchronize()
L.dbg_call("rbvae_dbg_jobs_stamps", None)
slots = st.cpu().numpy().reshape(SLOTS, CAP, 4)

print(f"launch: {'rbvae_run_jobs_sized' if a.sized else 'rbvae_run_jobs_table'}{', update table heaviest jobs first' if eng.jobs_heavy_first else ''}")
found = []
for s in slots:
    s = s[s[:, 0] > 0]
    if len(s):
        found.append(s)
for s in sorted(found, key=lambda s: s[:, 0].min()):
    tabs = [t for t in eng._tables.values() if t.block_map[1] == len(s)]
    t0, first_end = s[:, 0].min(), s[:, 1].min()
    rel = (s[:, :2] - t0) * 0.01
    late = s[:, 0] >= first_end
    print(f"\n{len(s)} workgroups, span {rel[:, 1].max():.1f} us, first workgroup ends at {(first_end - t0) * 0.01:.1f} us, "
          f"{int(late.sum())} workgroups start after it"
          + (f", LDS {J.job_lds_bytes(tabs[0].jl.rows)} bytes (sized launch: 36992)" if tabs else ""))
    if not tabs:
        continue
    t = tabs[0]
    bmap = t.block_map[0].cpu().numpy().reshape(-1, 4)
    kind = np.array([r[J.Col.KIND] for r in t.jl.rows])[bmap[s[:, 2], 0]]
    ctx = np.array([int(r[J.Col.INNER] != 0) for r in t.jl.rows])[bmap[s[:, 2], 0]]
    print(f"  {'kind':26s} {'wgs':>5s} {'first start':>11s} {'median start':>12s} {'last end':>9s} {'median life':>11s} {'start late':>10s}")
    for k in sorted(set(kind.tolist())):
        m = kind == k
        name = KINDS[k] + (" + adam" if k == 3 and ctx[m].any() else "")
        print(f"  {name:26s} {int(m.sum()):5d} {rel[m, 0].min():11.1f} {np.median(rel[m, 0]):12.1f} {rel[m, 1].max():9.1f} "
              f"{np.median(rel[m, 1] - rel[m, 0]):11.1f} {int(late[m].sum()):10d}")
