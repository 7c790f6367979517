"""Rows and uploaded tables of the batched job launches (rbvae_run_jobs, rbvae_run_jobs_sized).

A row is 16 x int64; include/rbvae_hip.h ("Batched layout jobs") is the authority on what each position means per job
kind.  This module is the one place that writes a row or reads one by position: `Col` names the positions, `JobList` has
a builder per kind, `JobTable` is a list uploaded to the device together with its block map.
"""
import struct
from enum import IntEnum
from typing import List

import numpy as np
import torch

from . import _lib as L

JOB_PACK, JOB_PERMUTE, JOB_ROWS, JOB_CONV_PACK, JOB_CONV_REDUCE, JOB_GATHER, JOB_ADAM_PACK, JOB_ADAM = range(8)

Col = IntEnum("Col", "KIND SRC DST D0 D1 D2 S0 S1 S2 NSLAB SLAB DTYPE ACCUMULATE SCALE_FAST INNER DST2", start=0)
DIMS, STRIDES = slice(Col.D0, Col.D2 + 1), slice(Col.S0, Col.S2 + 1)


def f32_bits(lo, hi=None):
    """The bits of one f32 (unsigned 32-bit), or of the pair (lo, hi) as one int64 with `lo` in the low word."""
    if hi is None:
        return struct.unpack("<I", struct.pack("<f", float(lo)))[0]
    return struct.unpack("<q", struct.pack("<ff", float(lo), float(hi)))[0]


def adam_context(flat, gflat, m, v, hyper, betas, eps, gscale):
    """Optimiser context of the fused update jobs (AdamCtx of csrc/jobs.hip), 8 x int64 on flat's device."""
    b1, b2 = betas
    return torch.tensor([flat.data_ptr(), gflat.data_ptr(), m.data_ptr(), v.data_ptr(), hyper.data_ptr(),
                         f32_bits(1.0 - b1, b2), f32_bits(1.0 - b2, eps), f32_bits(gscale, 0.0)], dtype=torch.int64).to(flat.device)


class JobList:
    """Rows of a job table, built kind by kind; every builder appends one row and returns it."""

    def __init__(self):
        self.rows: List[List[int]] = []
        self.keep = []          # tensors whose addresses the table holds

    def _row(self, kind, tensors, dims=(0, 0, 0), **cols):
        r = [0] * 16
        r[Col.KIND], r[DIMS] = kind, dims
        assert len(r) == 16, "dims has three entries"
        for name, val in cols.items():
            r[Col[name]] = int(val)
        self.rows.append(r)
        self.keep += tensors
        return r

    def add(self, kind, src, dst, dims, strides, nslab=1, slab=0, dtype=0, accumulate=0, scale=1.0):
        """Kinds 0 (pack), 1 (permute + reduce), 2 (reduce rows)."""
        # consecutive threads walk the index whose stride on the strided side is 1 (coalesced on that side;
        # the contiguous side then sees short strides that the caches absorb)
        fast = 2
        for ax in (2, 1, 0):
            if strides[ax] == 1 and dims[ax] > 1:
                fast = ax
                break
        # ... unless that index is the middle one of a long row with a short last index (conv weights): then a
        # thread walks the last index itself and both sides move in runs
        inner = kind in (JOB_PACK, JOB_PERMUTE) and fast == 1 and dims[2] <= 16 and dims[1] >= 64
        r = self._row(kind, [src, dst], dims, SRC=src.data_ptr(), DST=dst.data_ptr(), NSLAB=nslab, SLAB=slab, DTYPE=dtype,
                      ACCUMULATE=accumulate, SCALE_FAST=f32_bits(scale) | (fast << 32), INNER=inner)
        r[STRIDES] = strides
        assert len(r) == 16, "dims and strides have three entries each"
        return r

    def add_conv_pack(self, src, wf, wd, co, ci, kk, dtype):
        """f32 weight [co][ci][kk] -> [co][t][ci] (wf) and [ci][t][co] (wd) in one pass."""
        if kk > 16:
            raise ValueError("conv weight pack supports kernels up to 4x4")
        return self._row(JOB_CONV_PACK, [src, wf, wd], (co, ci, kk), SRC=src.data_ptr(), DST=wf.data_ptr(), NSLAB=1, DTYPE=dtype,
                         DST2=wd.data_ptr())

    def add_conv_reduce(self, slabs, dst, co, ci, kk, nslab, scale=1.0):
        """K-slice slabs [nslab][co][kk][ci] of a conv weight gradient -> torch layout [co][ci][kk], coalesced."""
        return self._row(JOB_CONV_REDUCE, [slabs, dst], (co, ci, kk), SRC=slabs.data_ptr(), DST=dst.data_ptr(), NSLAB=nslab,
                         SLAB=co * kk * ci, SCALE_FAST=f32_bits(scale))

    def add_gather(self, table, out, plan, counter=None):
        """out[r] = table[plan[counter % batches][r]]: table [rows][...] f32 (whole float4s per row), plan [batches][rows]."""
        keep = [t for t in (table, out, plan, counter) if t is not None]
        return self._row(JOB_GATHER, keep, (plan.shape[1], plan.shape[0], table[0].numel() // 4),
                         SRC=table.data_ptr(), DST=out.data_ptr(), S0=plan.data_ptr(), S1=0 if counter is None else counter.data_ptr(), S2=table.shape[0], NSLAB=1)

    def add_adam(self, src, ctx):
        """Kind 7: Adam update of the parameter tensor `src` (a view into the flat buffer of `ctx`), no packed copy."""
        return self._row(JOB_ADAM, [src, ctx], (src.numel(), 1, 1), SRC=src.data_ptr(), INNER=ctx.data_ptr())

    def add_adam_pack(self, ctx, a, b=None, what="job"):
        """Kind 6: Adam update of a tensor + the one or two packed copies that the kind-0 rows a, b would write.  The second
        copy's strides ride in NSLAB, SLAB, ACCUMULATE and its type in the second byte of DTYPE."""
        if b is None:
            b = [0] * 16
        elif b[DIMS] != a[DIMS]:
            raise RuntimeError(f"{what}: its two packed copies walk different logical shapes")
        r = self._row(JOB_ADAM_PACK, [ctx], a[DIMS], SRC=a[Col.SRC], DST=a[Col.DST], NSLAB=b[Col.S0], SLAB=b[Col.S1],
                      ACCUMULATE=b[Col.S2], DTYPE=a[Col.DTYPE] | (b[Col.DTYPE] << 8), INNER=ctx.data_ptr(), DST2=b[Col.DST])
        r[STRIDES] = a[STRIDES]
        return r

    def add_conv_pack_adam(self, row, ctx):
        """Kind 3 with the Adam context attached: the workgroups update the weight rows they pack."""
        return self._row(JOB_CONV_PACK, [ctx], row[DIMS], **{c.name: row[c] for c in (Col.SRC, Col.DST, Col.NSLAB, Col.DTYPE, Col.DST2)},
                         INNER=ctx.data_ptr())

    def upload(self, device):
        return torch.tensor(self.rows, dtype=torch.int64).to(device)

    def signature(self):
        return tuple(tuple(r) for r in self.rows)


def job_block_map(rows, device, cap):
    """Block map of a job table for rbvae_run_jobs_sized: one workgroup entry (job, index within the job, workgroups of the
    job) per workgroup the rows can use, at most `cap` per job.  -> (int32 device tensor [n][4], n)."""
    arr = np.ascontiguousarray(np.array(rows, dtype=np.int64).reshape(len(rows), 16))
    total = L.query("rbvae_job_block_map", arr.ctypes.data, len(rows), cap, None, 0)
    if total <= 0:
        raise RuntimeError("rbvae_job_block_map: " + L.lib().rbvae_last_error().decode())
    m = np.empty(4 * total, dtype=np.int32)
    if L.query("rbvae_job_block_map", arr.ctypes.data, len(rows), cap, m.ctypes.data, total) != total:
        raise RuntimeError("rbvae_job_block_map: " + L.lib().rbvae_last_error().decode())
    return torch.from_numpy(m).to(device), total


def job_lds_bytes(rows):
    """LDS of a launch of `rows` (rbvae_job_lds_bytes): the most any of its jobs touches, rounded up to 16 bytes."""
    arr = np.ascontiguousarray(np.array(rows, dtype=np.int64).reshape(len(rows), 16))
    n = L.query("rbvae_job_lds_bytes", arr.ctypes.data, len(rows))
    if n < 0:
        raise RuntimeError("rbvae_job_lds_bytes: " + L.lib().rbvae_last_error().decode())
    return n


def job_launch_order(rows, cap):
    """rbvae_job_launch_order: the permutation of the block map's entries that hands the heaviest jobs' entries out first
    (int32 numpy array)."""
    arr = np.ascontiguousarray(np.array(rows, dtype=np.int64).reshape(len(rows), 16))
    total = L.query("rbvae_job_block_map", arr.ctypes.data, len(rows), cap, None, 0)
    order = np.empty(max(total, 1), dtype=np.int32)
    if total <= 0 or L.query("rbvae_job_launch_order", arr.ctypes.data, len(rows), cap, order.ctypes.data, total) != total:
        raise RuntimeError("rbvae_job_launch_order: " + L.lib().rbvae_last_error().decode())
    return order


class JobTable:
    """A JobList on the device: `rows` (device tensor) and their count `n`, `block_map` = (map, workgroups) with at most
    `cap` workgroups per job; `jl` keeps the addressed tensors alive.  `host_rows` (the rows as the library reads them on
    the host), `cap` and `order` (rbvae_job_launch_order's permutation on the device) are what rbvae_run_jobs_table takes."""

    def __init__(self, jl: JobList, device, cap):
        self.jl, self.n, self.rows = jl, len(jl.rows), jl.upload(device)
        self.block_map = job_block_map(jl.rows, device, cap)
        self.cap = cap
        self.host_rows = np.ascontiguousarray(np.array(jl.rows, dtype=np.int64).reshape(self.n, 16))
        self.order = torch.from_numpy(job_launch_order(jl.rows, cap)).to(device)

    def run(self, heavy_first=False):
        """One launch of the table, sized by the library from the rows (rbvae_run_jobs_table)."""
        L.call("rbvae_run_jobs_table", self.host_rows.ctypes.data, self.n, self.cap, self.rows, self.block_map[0],
               self.order if heavy_first else None)
