"""Job tables of the rbvae_run_jobs_table tests (test_jobs_lds_cpu.py, test_jobs_lds_gpu.py): rows of every kind through the
JobList builders on real buffers, and a restatement of the highest LDS byte each branch of run_jobs_k touches, read off
the kernel's loops (csrc/jobs.hip), not off job_lds_bytes."""
from importlib import import_module

import torch

J = import_module("symbols-from-video_amd.jobs")
F32_T, BF16_T = 0, 1                       # RBVAE_F32 / RBVAE_BF16
CPK_MAXROW, CPK_CIB, CRD_CI, CPK_LDS_BYTES = 2304, 64, 256, 16 * (2304 + 8)

# name -> (kind, ...): the cases the tables are made of
CONV_PACKS = {                              # (co, ci, kk), type, with the Adam context
    "cpk_bf16_pieces": ((16, 128, 9), BF16_T, True),        # two pieces of 64 input channels
    "cpk_bf16_one_piece": ((16, 64, 9), BF16_T, True),
    "cpk_bf16_whole_row": ((8, 144, 16), BF16_T, False),    # 2 304 values per row: the limit
    "cpk_f32": ((8, 256, 9), F32_T, True),
    "cpk_scalar": ((5, 3, 9), BF16_T, False),               # no 16-byte path: ci % 8 != 0
}
SMALL = ("cpk_bf16_pieces", "cpk_bf16_one_piece", "cpk_f32", "rows_wave", "adam_flat", "adam_pack_flat", "gather")
ALL = tuple(CONV_PACKS) + ("conv_reduce", "rows_wide", "rows_wave", "adam_flat", "adam_pack_flat", "adam_tiled", "gather")
TILED = ("adam_tiled", "adam_flat", "gather")


def _ru(x, m):
    return (x + m - 1) // m * m


def lds_touched(r):
    """End of the highest LDS byte the workgroups of row r touch (0: none)."""
    kind, (d0, d1, d2) = r[J.Col.KIND], r[J.DIMS]
    if kind == J.JOB_CONV_PACK:             # tile[r * pitch + e]: r < NCO, e < the piece's row
        es = 4 if r[J.Col.DTYPE] == F32_T else 2
        nco = 16 // es
        cib = min((CPK_MAXROW // d2) // nco * nco, d1)
        if cib > CPK_CIB and d1 % CPK_CIB == 0:
            cib = CPK_CIB
        row = cib * d2
        pitch = _ru(row, 256 // es) + 8     # the same banks as the fixed pitch 2 312: a whole number of 256-byte bank rows + 8
        return ((nco - 1) * pitch + row) * es
    if kind == J.JOB_CONV_REDUCE:           # tile[tp * (cn + 1) + c]: tp < kk, c < cn, f32
        cn = min(CRD_CI, d1)
        return ((d2 - 1) * (cn + 1) + cn) * 4
    if kind == J.JOB_ROWS:                  # red[256] float4, wide rows only
        n = d0 * d1 * d2
        wide = r[J.Col.NSLAB] >= 1024 and n % 4 == 0 and r[J.Col.SLAB] % 4 == 0 and r[J.Col.SRC] % 16 == 0
        return 256 * 16 if wide else 0
    if kind == J.JOB_ADAM_PACK and d0 * d1 * d2 >= 1 << 20:      # tile[(l0 * T1 + l1) * (T2 + 1) + l2], f32
        fa = 0 if r[J.Col.S0] == 1 else (1 if r[J.Col.S1] == 1 else 2)
        fb = fa if not r[J.Col.DST2] else (0 if r[J.Col.NSLAB] == 1 else (1 if r[J.Col.SLAB] == 1 else 2))
        if fa == 2 and fb == 2:
            return 0
        if fa != 2 and fb != 2 and fa != fb:
            t0, t1, t2 = (32 if fb == 0 else 16), (32 if fb == 1 else 16), 16
        else:
            f = fa if fa != 2 else fb
            t0, t1, t2 = (32 if f == 0 else 8), (32 if f == 1 else 8), 32
        t0, t1, t2 = min(t0, d0), min(t1, d1), min(t2, d2)
        return ((t0 * t1 - 1) * (t2 + 1) + t2) * 4
    return 0


def table_lds(rows):
    return _ru(max(lds_touched(r) for r in rows), 16)


class Table:
    """The cases `names` as one JobList on `device`, with seeded inputs.  outputs: name -> tensor, everything a job writes."""

    def __init__(self, names, device, seed=7):
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=g).to(device)
        self.jl, self.outputs = J.JobList(), {}
        out = self.outputs
        # the optimiser's flat buffers: every context job's tensor is a 16-byte aligned slice of them
        sizes = {n: _ru(c[0][0] * c[0][1] * c[0][2], 4) for n, c in CONV_PACKS.items() if c[2]}
        sizes.update(adam_flat=1000, adam_pack_flat=_ru(5 * 7 * 3, 4), adam_tiled=32 * 256 * 128)
        sizes = {n: s for n, s in sizes.items() if n in names}
        total = max(sum(sizes.values()), 4)
        out["w"], self.grad, out["m"] = rnd(total) * 0.1, rnd(total) * 0.01, rnd(total) * 0.01
        out["v"] = (torch.rand(total, generator=g) * 1e-4).to(device)
        self.hyper = torch.tensor([2e-3, 0.97], device=device)
        ctx = J.adam_context(out["w"], self.grad, out["m"], out["v"], self.hyper, (0.9, 0.999), 1e-8, 0.5)
        at, view = 0, {}
        for n, s in sizes.items():
            view[n], at = out["w"][at:at + s], at + s
        plain = J.JobList()                  # the rows the fused jobs are made from
        for n in names:
            if n in CONV_PACKS:
                (co, ci, kk), dt, fused = CONV_PACKS[n]
                tdt = torch.float32 if dt == F32_T else torch.bfloat16
                wf, wd = torch.zeros(co * kk * ci, dtype=tdt, device=device), torch.zeros(ci * kk * co, dtype=tdt, device=device)
                out[n + "/wf"], out[n + "/wd"] = wf, wd
                if fused:
                    self.jl.add_conv_pack_adam(plain.add_conv_pack(view[n], wf, wd, co, ci, kk, dt), ctx)
                else:
                    self.jl.add_conv_pack(rnd(co * ci * kk), wf, wd, co, ci, kk, dt)
            elif n == "conv_reduce":         # two blocks of input channels (256 + 44), three slabs
                co, ci, kk, ns = 4, 300, 9, 3
                out[n] = torch.zeros(co * ci * kk, device=device)
                self.jl.add_conv_reduce(rnd(ns * co * kk * ci), out[n], co, ci, kk, ns, scale=0.5)
            elif n in ("rows_wide", "rows_wave"):
                ns, c = (1024, 8) if n == "rows_wide" else (16, 10)
                out[n] = torch.zeros(c, device=device)
                self.jl.add(J.JOB_ROWS, rnd(ns * c), out[n], (1, 1, c), (0, 0, 1), nslab=ns, slab=c, scale=0.25)
            elif n == "adam_flat":
                self.jl.add_adam(view[n][:1000], ctx)
            elif n == "adam_pack_flat":      # [5][7][3] -> bf16 [7][5][3]
                out[n] = torch.zeros(105, dtype=torch.bfloat16, device=device)
                self.jl.add_adam_pack(ctx, plain.add(J.JOB_PACK, view[n], out[n], (5, 7, 3), (3, 15, 1), dtype=BF16_T))
            elif n == "adam_tiled":          # 2^20 elements, the smallest tiled job: bf16 copy with i1 contiguous, f32 copy with i0
                d = (32, 256, 128)
                out[n + "/a"] = torch.zeros(1 << 20, dtype=torch.bfloat16, device=device)
                out[n + "/b"] = torch.zeros(1 << 20, device=device)
                a = plain.add(J.JOB_PACK, view[n], out[n + "/a"], d, (256 * 128, 1, 256), dtype=BF16_T)
                b = plain.add(J.JOB_PACK, view[n], out[n + "/b"], d, (1, 32 * 128, 32), dtype=F32_T)
                self.jl.add_adam_pack(ctx, a, b)
            elif n == "gather":              # 6 rows of 3 float4 out of a table of 11, batch 3 of 5 (counter 13)
                table = rnd(11, 2, 3, 2)
                plan = torch.randint(0, 11, (5, 6), generator=g).to(device)
                out[n] = torch.zeros(6, 12, device=device)
                self.jl.add_gather(table, out[n], plan, torch.tensor([13], dtype=torch.int64, device=device))
            else:
                raise KeyError(n)
        assert len(self.jl.rows) == len(names)
