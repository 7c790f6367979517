"""CPU: the LDS a job launch is given (rbvae_job_lds_bytes, what rbvae_run_jobs_table sizes its launch with; pure host
code over the geometry functions of csrc/jobs.hip) against a restatement of the highest byte every branch of run_jobs_k
touches (tests/_jobs_lds_cases.py), row by row and per table; and rbvae_job_launch_order, the optional order in which a
launch's workgroups take the block map's entries."""
from importlib import import_module

import numpy as np
import pytest

import _jobs_lds_cases as K
import sfv_amd

J = import_module("symbols-from-video_amd.jobs")

# the figures by hand, from the kernel's index expressions
BY_HAND = {
    "cpk_bf16_pieces": (7 * 648 + 576) * 2,         # 8 rows of 576 bf16 at pitch 5 * 128 + 8
    "cpk_bf16_one_piece": (7 * 648 + 576) * 2,
    "cpk_bf16_whole_row": (7 * 2312 + 2304) * 2,    # the fixed pitch at the limit
    "cpk_f32": (3 * 584 + 576) * 4,                 # 4 rows of 64 channels x 9 f32 at pitch 9 * 64 + 8
    "cpk_scalar": (7 * 136 + 27) * 2,
    "conv_reduce": (8 * 257 + 256) * 4,
    "rows_wide": 4096, "rows_wave": 0, "adam_flat": 0, "adam_pack_flat": 0, "gather": 0,
    "adam_tiled": (511 * 17 + 16) * 4,              # [32 * 16][16 + 1] f32
}


@pytest.fixture(scope="module")
def table():
    return K.Table(K.ALL, "cpu")


def test_every_row_gets_the_bytes_its_branch_touches(table):
    assert set(BY_HAND) == set(K.ALL)
    for name, r in zip(K.ALL, table.jl.rows):
        want = K.lds_touched(r)
        assert want == BY_HAND[name], name
        assert J.job_lds_bytes([r]) == (want + 15) // 16 * 16, name


@pytest.mark.parametrize("names", [K.ALL, K.SMALL, K.TILED, ("gather", "adam_flat"), ("rows_wide", "rows_wave")])
def test_a_table_gets_the_maximum_over_its_jobs(table, names):
    rows = [table.jl.rows[K.ALL.index(n)] for n in names]
    got = J.job_lds_bytes(rows)
    assert got == K.table_lds(rows) == max(J.job_lds_bytes([r]) for r in rows)
    assert got % 16 == 0 and got <= K.CPK_LDS_BYTES
    assert got == {K.ALL: 36976, K.SMALL: 10224, K.TILED: 34816}.get(names, got)


def test_bank_rule_of_the_conv_pack_pitch():
    """The pitch of every staged row is the fixed pitch 2 312 modulo the 256-byte bank row, so no element changes its bank."""
    for es in (2, 4):
        for row in range(4, K.CPK_MAXROW + 1, 4):
            pitch = K._ru(row, 256 // es) + 8
            assert pitch >= row + 8 and (pitch * es) % 256 == ((K.CPK_MAXROW + 8) * es) % 256
        assert K._ru(K.CPK_MAXROW, 256 // es) + 8 == K.CPK_MAXROW + 8


def test_refusals():
    L = sfv_amd._lib
    assert L.query("rbvae_job_lds_bytes", None, 1) < 0
    arr = np.zeros((1, 16), dtype=np.int64)
    assert L.query("rbvae_job_lds_bytes", arr.ctypes.data, 0) < 0
    assert L.query("rbvae_job_launch_order", arr.ctypes.data, 1, 256, None, 1) < 0
    rows = np.array(K.Table(("gather",), "cpu").jl.rows, dtype=np.int64)       # 6 workgroups
    order = np.full(8, -7, dtype=np.int32)
    assert L.query("rbvae_job_launch_order", rows.ctypes.data, 1, 256, order.ctypes.data, 5) < 0
    assert order.tolist() == [-7] * 8


@pytest.mark.parametrize("cap", [3, 256])
def test_launch_order_is_a_bijection_and_a_function_of_the_rows(table, cap):
    rows = table.jl.rows
    arr = np.ascontiguousarray(np.array(rows, dtype=np.int64))
    total = sfv_amd._lib.query("rbvae_job_block_map", arr.ctypes.data, len(rows), cap, None, 0)
    order = J.job_launch_order(rows, cap)
    assert len(order) == total and sorted(order.tolist()) == list(range(total))
    assert np.array_equal(order, J.job_launch_order([list(r) for r in rows], cap))
    # another table with the same dimensions at other addresses: the same order
    other = K.Table(K.ALL, "cpu", seed=8).jl.rows
    assert np.array_equal(order, J.job_launch_order(other, cap))
    # the entries of a job stay together and in their order; a job with more bytes per workgroup never comes later
    m = np.empty(4 * total, dtype=np.int32)
    assert sfv_amd._lib.query("rbvae_job_block_map", arr.ctypes.data, len(rows), cap, m.ctypes.data, total) == total
    m = m.reshape(-1, 4)[order]
    jobs_in_order = [int(j) for i, j in enumerate(m[:, 0]) if i == 0 or j != m[i - 1, 0]]
    assert sorted(jobs_in_order) == list(range(len(rows)))
    for j in range(len(rows)):
        assert m[m[:, 0] == j, 1].tolist() == list(range(int((m[:, 0] == j).sum())))
    first = K.ALL[jobs_in_order[0]]
    assert first == "adam_tiled", first                 # 8 192 elements x 32 bytes per workgroup
