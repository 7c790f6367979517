"""CPU: the job tables' two host-side halves against the tests' own restatement of the row format (tests/_layout_cases.py,
tests/_loss_cases.py, and the literal rows of test_loss_bounds_gpu.py repeated below).

  rbvae_job_block_map (csrc/jobs.hip, pure host code; sized from the geometry functions the kernel's loops run over) equals
  _layout_cases.block_map entry for entry on one table that holds a row of every branch of run_jobs_k.
  Every JobList builder (symbols-from-video_amd/jobs.py) gives, position by position, the row the restatement gives.

Only dimensions, strides and pointer alignment reach the block map, so the table's pointers are small aligned integers."""
import ctypes
import struct
from importlib import import_module

import numpy as np
import pytest
import torch

import _layout_cases as C
import _loss_cases as LC
import sfv_amd

J = import_module("symbols-from-video_amd.jobs")
F32_T, BF16_T = C.F32_T, C.BF16_T
CP = 1 << 20                                    # the "pointer" of the optimiser context in the rows below


def update_row(j, src, dsts, cp=CP):
    """Row of a fused-update job (_loss_cases.job), the literal form of test_loss_bounds_gpu._run_table."""
    d0, d1, d2 = j["dims"]
    if j["kind"] == 7:
        return [7, src, 0, d0 * d1 * d2, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, cp, 0]
    if j["kind"] == 3:
        return [3, src, dsts[0], d0, d1, d2, 0, 0, 0, 1, 0, j["dtype"], 0, 0, cp, dsts[1]]
    two = len(j["copies"]) == 2
    (t1, a), (t2, b) = j["copies"][0], (j["copies"][1] if two else (0, (0, 0, 0)))
    return [6, src, dsts[0], d0, d1, d2, a[0], a[1], a[2], b[0], b[1], t1 | (t2 << 8), b[2], 0, cp, dsts[1] if two else 0]


def every_branch_table():
    rows = [C.table_row(kind, c, dt, src=4096 * (i + 1), dst=4096 * (i + 1) + 1024, dst2=4096 * (i + 1) + 2048, plan=64, counter=128)
            for i, (kind, c, dt) in enumerate(C.table_jobs())]
    for jobs in LC.JOB_TABLES.values():
        rows += [update_row(j, 16 * (len(rows) + i), (32, 48)) for i, j in enumerate(jobs)]
    return rows


def lib_block_map(rows, cap, capacity=None):
    """(return value of the counting call, return value of the writing call, the map as a list) of rbvae_job_block_map."""
    L = sfv_amd._lib
    arr = np.ascontiguousarray(np.array(rows, dtype=np.int64).reshape(len(rows), 16))
    total = L.query("rbvae_job_block_map", arr.ctypes.data, len(rows), cap, None, 0)
    capacity = total if capacity is None else capacity
    m = np.full(4 * max(capacity, 1) + 4, -7, dtype=np.int32)                 # one guard entry behind the map
    got = L.query("rbvae_job_block_map", arr.ctypes.data, len(rows), cap, m.ctypes.data, capacity)
    assert m[4 * max(capacity, 1):].tolist() == [-7] * 4, "the map writer wrote past its capacity"
    return total, got, m[:4 * capacity].reshape(-1, 4).tolist()


def test_table_holds_every_branch():
    want = {b for b in C.LAYOUT_BRANCHES if b.startswith("run_jobs_k")} | set(LC.JOB_BRANCHES)
    assert {C.job_branch(r) for r in every_branch_table()} == want
    assert {f"run_jobs_k[6,tiled,{c}]" for c in ("one", "same", "different", "mixed")} <= want


@pytest.mark.parametrize("cap", [3, 256, 65535])
def test_library_block_map_equals_the_restatement(cap):
    rows = every_branch_table()
    want = C.block_map(rows, cap)
    total, got, m = lib_block_map(rows, cap)
    assert total == len(want), "the count-only call (map_host == NULL)"
    assert got == len(want)
    for i, (a, b) in enumerate(zip(m, want)):
        assert a == b, f"cap {cap}: map entry {i} is {a}, the restated job_blocks_of gives {b} ({C.job_branch(rows[b[0]])})"
    # per job: the workgroups the library gives each row, against the restatement (names the branch that differs)
    per_job = np.bincount(np.array(m)[:, 0], minlength=len(rows)).tolist()
    assert per_job == [min(max(C.job_blocks_of(r), 1), cap) for r in rows]


def test_block_map_refuses_a_capacity_one_short():
    rows = every_branch_table()
    total, got, _ = lib_block_map(rows, 256, capacity=len(C.block_map(rows, 256)) - 1)
    assert total == len(C.block_map(rows, 256)) and got < 0
    assert "too small" in sfv_amd._lib.lib().rbvae_last_error().decode()


# ---- the builders ------------------------------------------------------------------------------------------------------------------------

def _t(n=64, dtype=torch.float32):
    return torch.zeros(n, dtype=dtype)


def _same(got, want, what):
    assert len(got) == len(want) == 16
    for col, (a, b) in zip(J.Col, zip(got, want)):
        assert a == b and type(a) is int, f"{what}: column {col.name} is {a!r}, the restated row has {b!r}"


def test_generic_builder_equals_the_restated_row():
    jl = J.JobList()
    src, dst = _t(), _t()
    p, q = src.data_ptr(), dst.data_ptr()
    cases = [  # the first three rows of test_job_blocks_of_literals (fast / inner: 1/0, 1/1, 2/0), then every keyword
        (0, (5, 7, 9), (63, 1, 7), {}), (0, (5, 64, 9), (576, 1, 64), dict(dtype=BF16_T)),
        (1, (9, 10, 5), (5, 45, 1), dict(nslab=3, slab=450)), (1, (4, 64, 9), (576, 1, 64), dict(nslab=5, slab=2304, accumulate=1, scale=-0.25)),
        (1, (6, 3, 1), (1, 6, 0), dict(nslab=2, slab=18, scale=0.5)), (2, (1, 1, 64), (0, 0, 1), dict(nslab=2049, slab=64, accumulate=1, scale=3.0)),
    ]
    for kind, dims, strides, kw in cases:
        got = jl.add(kind, src, dst, dims, strides, **kw)
        kw = {("acc" if k == "accumulate" else k): v for k, v in kw.items()}
        _same(got, C.job_row(kind, p, q, dims, strides, **kw), f"add kind {kind} {dims}")
        assert jl.rows[-1] is got
    assert [(r[J.Col.SCALE_FAST] >> 32, r[J.Col.INNER]) for r in jl.rows[:3]] == [(1, 0), (1, 1), (2, 0)]
    assert jl.signature() == tuple(tuple(r) for r in jl.rows) and len(jl.rows) == len(cases)


def test_conv_and_gather_builders_equal_the_restated_rows():
    jl = J.JobList()
    src, wf, wd = _t(), _t(64, torch.bfloat16), _t(64, torch.bfloat16)
    _same(jl.add_conv_pack(src, wf, wd, 8, 328, 9, BF16_T),
          C.job_row(3, src.data_ptr(), wf.data_ptr(), (8, 328, 9), dtype=BF16_T, dst2=wd.data_ptr()), "add_conv_pack")
    with pytest.raises(ValueError):
        jl.add_conv_pack(src, wf, wd, 8, 8, 25, BF16_T)
    _same(jl.add_conv_reduce(src, wd, 3, 520, 9, 2, scale=0.5),
          C.job_row(4, src.data_ptr(), wd.data_ptr(), (3, 520, 9), nslab=2, slab=3 * 9 * 520, scale=0.5), "add_conv_reduce")
    table, plan, out, counter = torch.zeros(11, 2, 3, 4), torch.zeros(5, 3, dtype=torch.int64), _t(), torch.zeros(1, dtype=torch.int64)
    for cnt in (counter, None):                   # dims = (rows of a batch, batches, float4 per row); strides = (plan, counter, table rows)
        want = C.job_row(5, table.data_ptr(), out.data_ptr(), (3, 5, 6), (plan.data_ptr(), cnt.data_ptr() if cnt is not None else 0, 11))
        want[9] = 1           # the trainer's gather row has always carried nslab = 1 (no branch reads it); job_row leaves it 0
        _same(jl.add_gather(table, out, plan, cnt), want, "add_gather")
    assert len(jl.rows) == 4


def test_adam_builders_equal_the_literal_rows():
    jl, packs = J.JobList(), J.JobList()
    flat, ctx = _t(4096), torch.zeros(8, dtype=torch.int64)
    src, cp = flat[128:128 + 1000], ctx.data_ptr()
    _same(jl.add_adam(src, ctx), update_row(LC.job("b", 7, (1000, 1, 1)), src.data_ptr(), (), cp), "add_adam")
    _same(jl.add_adam(src, ctx), [7, src.data_ptr(), 0, 1000, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, cp, 0], "add_adam, written out")
    # kind 6 from the kind-0 rows it replaces: one copy, then two copies of different types
    da, db = _t(64, torch.bfloat16), _t()
    for j in (LC.j6("one", (5, 7, 3), (BF16_T, (2, 1, 0))), LC.j6("two", (7, 11, 13), (F32_T, (1, 2, 0)), (BF16_T, (2, 1, 0))),
              LC.j6("two'", (33, 20, 1), (BF16_T, (0, 1, 2)), (F32_T, (1, 0, 2)))):
        rows0 = [packs.add(J.JOB_PACK, src, d, j["dims"], s, dtype=dt) for d, (dt, s) in zip((da, db), j["copies"])]
        _same(jl.add_adam_pack(ctx, *rows0, what=j["id"]), update_row(j, src.data_ptr(), (da.data_ptr(), db.data_ptr()), cp), "add_adam_pack " + j["id"])
    a = packs.add(J.JOB_PACK, src, da, (7, 11, 13), (1, 7, 77), dtype=BF16_T)
    b = packs.add(J.JOB_PACK, src, db, (7, 13, 11), (1, 7, 91))
    n = len(jl.rows)
    with pytest.raises(RuntimeError, match="fc.weight: its two packed copies walk different logical shapes"):
        jl.add_adam_pack(ctx, a, b, what="fc.weight")
    assert len(jl.rows) == n
    # kind 3 with the context attached; the row it came from is left alone
    wf, wd = _t(64, torch.bfloat16), _t(64, torch.bfloat16)
    plain = packs.add_conv_pack(src, wf, wd, 16, 144, 16, BF16_T)
    _same(jl.add_conv_pack_adam(plain, ctx), update_row(LC.job("c", 3, (16, 144, 16), BF16_T), src.data_ptr(), (wf.data_ptr(), wd.data_ptr()), cp),
          "add_conv_pack_adam")
    assert plain[J.Col.INNER] == 0


def test_adam_context_and_f32_bits():
    f2 = lambda a, b: struct.unpack("<q", struct.pack("<ff", float(a), float(b)))[0]       # test_loss_bounds_gpu._f2
    bufs = [_t(8) for _ in range(5)]
    ctx = J.adam_context(*bufs, (0.9, 0.999), 1e-8, 0.5)
    assert ctx.dtype == torch.int64 and ctx.tolist() == [t.data_ptr() for t in bufs] + [f2(1.0 - 0.9, 0.999), f2(1.0 - 0.999, 1e-8), f2(0.5, 0.0)]
    assert J.f32_bits(1.0) == 0x3F800000 and J.f32_bits(-2.0) == 0xC0000000 and J.f32_bits(1.0, -2.0) == ctypes.c_int64(0xC00000003F800000).value
    assert [c.value for c in J.Col] == list(range(16))
