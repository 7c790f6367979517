"""Element-wise float64 bounds, exact copies and guarded stores for the layout, reduce and job kernels (tests/_layout_cases.py
holds the cases, the float64 references, the derived summation heights, the f32 emulations and the dispatch restatements;
tests/_bounds.py the buffers).  Entry points this file calls (the last test asserts that each of them was):

  csrc/layout.hip   rbvae_pack3, rbvae_permute_reduce, rbvae_cast_pad, rbvae_colsum, rbvae_colsum_partial,
                    rbvae_colsum_ws_floats, rbvae_reduce_rows, rbvae_skinny_linear, rbvae_skinny_linear_parts,
                    rbvae_gather_frames
  csrc/jobs.hip     rbvae_run_jobs, rbvae_run_jobs_sized, rbvae_job_block_map: kinds 0-5 in one mixed table (every branch of
                    _layout_cases.LAYOUT_BRANCHES), launched with 1, 3 and 256 workgroups per job and with block maps capped at 2
                    and 65535 -- bit-identical outputs, and with accumulate = 0 bit-equal to the direct entry points
  csrc/eval.hip     rbvae_state_vote

Every output sits inside NaN sentinels (assert_guards / assert_guards_where after every launch: no stray store, every declared
element written, gaps of a strided destination untouched); every strided input carries NaN in its padding, its gaps and its
guard rows.  Sums are checked element by element against float64 with the bound |scale| h u sum|v| + u |ref| (+ u |prev + ref|),
h the summation height of the branch; packs, casts and gathers bit for bit; the vote as integers.  Refusals return the error,
rbvae_last_error names the entry point, and nothing is written.

Worst |err| / bound per quantity, measured on one MI355X (every case prints its own as BOUNDS ... worst |err|/bound):
    pack3, cast_pad, gather_frames (gx = 1, 4, 8), state_vote, job kinds 0, 3 (every branch) and 5: exact
    permute_reduce 0.704   reduce_rows 0.465
    colsum_partial_k<f32> partial rows 0.299, colsum 0.108     colsum_partial_k<bf16> partial rows exact, colsum 0.213
    colsum_partial_vec_k<f32> partial rows 0.374, colsum 0.083  colsum_partial_vec_k<bf16> partial rows exact, colsum 0.032
    skinny_linear_k f32 0.097, bf16 0.055, parts f32 0.110, parts bf16 0.023
    run_jobs_k  [1,fast0] 0.258  [1,fast1] 0.476  [1,fast2] 0.391  [1,inner] 0.397  [1,inner,4slabs] 0.348  [2,wave] 0.056
                [2,wide] 0.012  [4,na1] 0.562  [4,na3] 0.704  [4,na4] 0.654  [4,na3,ncb] 0.389  [4,na1,ncb] 0.572
(the partial rows of bf16 inputs are exact because at most 32 eight-bit significands meet in one f32 chain).  The five launch
shapes of the mixed table agreed bit for bit, and so did the jobs with accumulate = 0 and their direct entry points; no
kernel defect turned up.  Without a device (test_layout_bounds_cpu.py): an f32 emulation of every operation passes every bound
(sums at 0.06 - 0.7 of it), every summand is at least 23 bounds large, and each of the 23 named defects fails."""
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import _bounds as B
import _layout_cases as C
import rbvae_oracle as O

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
F32_T, BF16_T = C.F32_T, C.BF16_T
ids = lambda cases: [c["id"] for c in cases]
CALLED = set()


@pytest.fixture(scope="module")
def lib():
    import sfv_amd
    return sfv_amd._lib


def call(lib, name, *args):
    CALLED.add(name)
    try:
        lib.call(name, *args)
        torch.cuda.synchronize()
    except RuntimeError as e:                                   # a launch or device error: launch nothing more on this device
        pytest.exit(f"{name}: {e}", returncode=3)


def report(kind, c, res):
    res = " ".join(f"{k} {v:.3g}" for k, v in res.items()) if isinstance(res, dict) else f"{res:.3g}"
    print(f"\nBOUNDS {kind} {c} worst |err|/bound = {res}")


def flat(t, dtype=F32):
    """A contiguous input (or preloaded output) of any length inside NaN guards."""
    g = B.GuardedFlat(t.numel(), dtype)
    g.view.copy_(t.reshape(-1).to(dtype))
    return g


def flat_out(n, prev=None, dtype=F32):
    g = B.GuardedFlat(n, dtype)
    if prev is not None:
        g.view.copy_(prev.reshape(-1))
    return g


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32).cpu()


def untouched(*gs):
    for g in gs:
        ib, pat = B.SENTINEL[g.dtype]
        assert bool((g.buf.view(ib) == pat).all()), "a refused call wrote to its output"


def counter_dev(value):
    """A device uint64 between two sentinels; (buffer, pointer to the middle element or None)."""
    if value is None:
        return None, None
    buf = torch.tensor([0x5EED5EED, value - (1 << 64) if value >= (1 << 63) else value, 0x5EED5EED], dtype=torch.int64, device="cuda")
    return buf, buf.data_ptr() + 8


# ---- pack3, permute_reduce, cast_pad ---------------------------------------------------------------------------------------------------

def direct_pack(lib, c, dt, src):
    out = B.GuardedFlat(C.pack_span(c), C.TDT[dt])
    call(lib, "rbvae_pack3", dt, src.view, out.view, *c["dims"], *c["strides"])
    written = torch.zeros(C.pack_span(c), dtype=torch.bool)
    written[C.idx3(c["dims"], c["strides"])] = True
    B.assert_guards_where(out, written, f"pack3 {c['id']}")
    return out.view.cpu()


@pytest.mark.parametrize("dt", [F32_T, BF16_T], ids=["f32", "bf16"])
@pytest.mark.parametrize("c", C.PACK_CASES, ids=ids(C.PACK_CASES))
def test_pack3_exact_and_guarded(lib, c, dt):
    x = C.pack_data(c)
    got = direct_pack(lib, c, dt, flat(x))
    report("pack3", f"{c['id']}-{C.DTN[dt]}", C.check_pack(c, x, dt, got, c["id"]))


def direct_reduce(lib, c, src, prev):
    out = flat_out(C.numel(c["dims"]), prev)
    call(lib, "rbvae_permute_reduce", src.view, c["nslab"], c["slab"], out.view, *c["dims"], *c["strides"], c["scale"], c["acc"])
    B.assert_guards(out, f"permute_reduce {c['id']}")
    return out.view.cpu()


@pytest.mark.parametrize("c", C.PERMUTE_CASES + C.CONVRED_CASES, ids=ids(C.PERMUTE_CASES + C.CONVRED_CASES))
def test_permute_reduce_bounded_and_guarded(lib, c):
    d = C.reduce_data(c)
    got = direct_reduce(lib, c, flat(d[0]), d[1])
    report("permute_reduce", c["id"], C.check_sum(got, C.reduce_model(c, d), c["id"]))


@pytest.mark.parametrize("c", C.CASTPAD_CASES, ids=ids(C.CASTPAD_CASES))
def test_cast_pad_exact_and_guarded(lib, c):
    x = C.castpad_data(c)
    src, out = flat(x), B.GuardedFlat(c["rows"] * c["Lpad"], C.TDT[c["dt"]])
    call(lib, "rbvae_cast_pad", c["dt"], src.view, out.view, c["rows"], c["L"], c["Lpad"])
    B.assert_guards(out, c["id"])
    report("cast_pad", c["id"], C.check_castpad(c, x, out.view.cpu().view(c["rows"], c["Lpad"]), c["id"]))


# ---- column sums ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", C.COLSUM_CASES, ids=ids(C.COLSUM_CASES))
def test_colsum_bounded_and_guarded(lib, c):
    P, Cn, ld, es, xo, wo = c["P"], c["C"], c["ld"], C.ES[c["dt"]], c["xoff"], c["wsoff"]
    d = C.colsum_data(c)
    X = B.guarded(P, ld, Cn + xo, C.TDT[c["dt"]], row_align=es)
    X.view[:, xo:xo + Cn] = d[0].to(C.TDT[c["dt"]]).cuda()
    xp = X.view.data_ptr() + xo * es
    nws = lib.query("rbvae_colsum_ws_floats", P, Cn)
    CALLED.add("rbvae_colsum_ws_floats")
    assert nws == C.colsum_ws_floats(P, Cn)
    declared = torch.arange(nws + wo) >= wo
    res = {}
    ws = B.GuardedFlat(nws + wo, F32)
    call(lib, "rbvae_colsum_partial", c["dt"], xp, P, Cn, ld, ws.view.data_ptr() + 4 * wo)
    B.assert_guards_where(ws, declared, c["id"] + " partial")
    res["partial"] = C.check_sum(ws.view.cpu()[wo:].view(-1, Cn), C.partial_model(c, d[0]), c["id"] + " partial", ("block", "column"))
    ws2, out = B.GuardedFlat(nws + wo, F32), flat_out(Cn, d[1])
    call(lib, "rbvae_colsum", c["dt"], xp, P, Cn, ld, out.view, ws2.view.data_ptr() + 4 * wo, c["scale"], c["acc"])
    B.assert_guards_where(ws2, declared, c["id"] + " workspace")
    B.assert_guards(out, c["id"])
    assert torch.equal(bits(ws2.view), bits(ws.view)), "rbvae_colsum's partial rows differ from rbvae_colsum_partial's"
    res["colsum"] = C.check_sum(out.view.cpu(), C.colsum_model(c, d), c["id"])
    report(C.colsum_branch(c), c["id"], res)


@pytest.mark.parametrize("c", C.REDUCE_ROWS_CASES, ids=ids(C.REDUCE_ROWS_CASES))
def test_reduce_rows_bounded_and_guarded(lib, c):
    d = C.reduce_rows_data(c)
    ws, out = flat(d[0]), flat_out(c["C"], d[1])
    call(lib, "rbvae_reduce_rows", ws.view, c["rows"], c["C"], out.view, c["scale"], c["acc"])
    B.assert_guards(out, c["id"])
    report("reduce_rows", c["id"], C.check_sum(out.view.cpu(), C.reduce_rows_model(c, d), c["id"]))


# ---- skinny_linear ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", C.SKINNY_CASES, ids=ids(C.SKINNY_CASES))
def test_skinny_linear_bounded_and_guarded(lib, c):
    A, Bm, bias = C.skinny_data(c)
    t = C.TDT[c["dt"]]
    a, b = B.poisoned(A, c["lda"], t), B.poisoned(Bm, c["ldb"], t)
    bv = flat(bias) if bias is not None else None
    rows = c["ksplit"] * c["M"]
    out = B.guarded(rows, c["ldo"], c["Nc"], F32, row_align=4)
    args = [c["dt"], a.view, b.view, bv.view if bv else None, out.view, c["M"], c["Nc"], c["K"], c["lda"], c["ldb"], c["ldo"]]
    if c["ksplit"] > 1:
        call(lib, "rbvae_skinny_linear_parts", *args, c["ksplit"])
    else:
        call(lib, "rbvae_skinny_linear", *args)
    B.assert_guards(out, c["id"])
    got = out.buf[out.g:out.g + rows + C.SKINNY_TAIL].cpu()           # the rows behind the last part are guard rows
    report(C.skinny_branch(c), c["id"], C.check_skinny(c, (A, Bm, bias), got, c["id"]))


# ---- gather_frames ------------------------------------------------------------------------------------------------------------------------

def gather_inputs(c):
    table, plan = C.gather_data(c)
    tab = B.guarded(c["table_rows"], c["fe"], c["fe"], F32, guard_rows=1)
    tab.view.view(torch.int32).copy_(table)
    cbuf, cptr = counter_dev(c["counter"])
    return dict(data=(table, plan), table=tab, plan=plan.cuda().contiguous(), cbuf=cbuf, cptr=cptr)


def direct_gather(lib, c, gi):
    out = B.GuardedFlat(c["rows"] * c["fe"], F32)
    call(lib, "rbvae_gather_frames", gi["table"].view, c["table_rows"], gi["plan"], c["rows"], c["nb"], gi["cptr"], c["fe"], out.view)
    B.assert_guards(out, c["id"])
    if gi["cbuf"] is not None:
        v = gi["cbuf"].cpu().tolist()
        assert v[0] == v[2] == 0x5EED5EED and v[1] % (1 << 64) == c["counter"], "the gather changed the device counter"
    return out.view.view(torch.int32).cpu().view(c["rows"], c["fe"])


@pytest.mark.parametrize("c", C.GATHER_CASES, ids=ids(C.GATHER_CASES))
def test_gather_frames_exact_and_guarded(lib, c):
    gi = gather_inputs(c)
    report(f"gather_frames_k[gx={C.gather_gx(c['fe'])}]", c["id"], C.check_gather(c, gi["data"], direct_gather(lib, c, gi), c["id"]))


# ---- state_vote ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", C.VOTE_CASES, ids=ids(C.VOTE_CASES))
def test_state_vote_exact_and_guarded(lib, c):
    codes, labels = C.vote_data(c)
    cd, lab = flat(codes), labels.cuda()
    keys, counts, out = B.GuardedFlat(4 * c["F"], F32), B.GuardedFlat(c["F"], F32), B.GuardedFlat(2 * c["n_states"], F32)
    call(lib, "rbvae_state_vote", cd.view, lab, c["F"], c["L"], c["n_states"], keys.view, counts.view, out.view)
    for g in (keys, counts, out):
        B.assert_guards(g, c["id"])
    got = {k: g.view.view(torch.int32).cpu().numpy() for k, g in (("keys", keys), ("counts", counts), ("out", out))}
    C.check_vote(c, (codes, labels), got, c["id"])
    with np.errstate(invalid="ignore"):
        binary = (codes.numpy() > 0.5).astype(np.float32)
    avg, pct = O.state_consistency(binary, labels.numpy(), c["n_states"])
    mine = C.vote_consistency(c, got["out"])
    assert mine[1] == pytest.approx(pct, abs=1e-12) and mine[0] == pytest.approx(avg, abs=1e-12)
    report("state_vote", c["id"], 0.0)


# ---- the mixed job table, five launch shapes ------------------------------------------------------------------------------------------------

LAUNCHES = [("blocks", 1), ("blocks", 3), ("blocks", 256), ("sized", 2), ("sized", 65535)]


def table_inputs():
    """Device inputs of every job of the mixed table, built once."""
    out = []
    for kind, c, dt in C.table_jobs():
        e = dict(kind=kind, c=c, dt=dt, prev=None)
        if kind == 0:
            e["data"] = C.pack_data(c)
            e["src"] = flat(e["data"])
        elif kind in (1, 4):
            e["data"] = C.reduce_data(c)
            e["src"], e["prev"] = flat(e["data"][0]), e["data"][1]
        elif kind == 2:
            e["data"] = C.rows2_data(c)
            t = torch.full((c["nslab"] * c["slab"] + 4,), float("nan"))
            t[c["soff"]:c["soff"] + c["nslab"] * c["slab"]] = e["data"][0].reshape(-1)
            e["src"], e["prev"] = flat(t), e["data"][1]
        elif kind == 3:
            e["data"] = C.convpack_data(c)
            e["src"] = flat(e["data"])
        else:
            e.update(gather_inputs(c))
            e["src"] = e["table"]
        out.append(e)
    return out


def table_outputs(e):
    kind, c = e["kind"], e["c"]
    if kind == 0:
        return [B.GuardedFlat(C.pack_span(c), C.TDT[e["dt"]])]
    if kind in (1, 4):
        return [flat_out(C.numel(c["dims"]), e["prev"])]
    if kind == 2:
        return [flat_out(c["n"], e["prev"])]
    if kind == 3:
        return [B.GuardedFlat(C.numel(c["dims"]), C.TDT[e["dt"]]) for _ in range(2)]
    return [B.GuardedFlat(c["rows"] * c["fe"], F32)]


def run_table(lib, entries, how, arg):
    outs = [table_outputs(e) for e in entries]
    rows = []
    for e, o in zip(entries, outs):
        rows.append(C.table_row(e["kind"], e["c"], e["dt"], src=e["src"].view.data_ptr(), dst=o[0].view.data_ptr(),
                                dst2=o[1].view.data_ptr() if len(o) > 1 else 0,
                                plan=e["plan"].data_ptr() if e["kind"] == 5 else 0, counter=(e["cptr"] or 0) if e["kind"] == 5 else 0))
    tab = torch.tensor(rows, dtype=torch.int64).cuda()
    if how == "sized":
        E = import_module("symbols-from-video_amd.engine")
        bmap, nb = E.job_block_map(rows, torch.device("cuda", 0), arg)
        CALLED.add("rbvae_job_block_map")
        want = C.block_map(rows, arg)
        assert nb == len(want) and bmap.cpu().view(-1, 4).tolist() == want, "rbvae_job_block_map differs from the restated job_blocks_of"
        call(lib, "rbvae_run_jobs_sized", tab, bmap, nb)
    else:
        call(lib, "rbvae_run_jobs", tab, len(rows), arg)
    for e, o in zip(entries, outs):
        what = f"{how} {arg}: kind {e['kind']} {e['c']['id']}"
        if e["kind"] == 0:
            written = torch.zeros(C.pack_span(e["c"]), dtype=torch.bool)
            written[C.idx3(e["c"]["dims"], e["c"]["strides"])] = True
            B.assert_guards_where(o[0], written, what)
        else:
            for g in o:
                B.assert_guards(g, what)
    return rows, [[g.view.cpu() for g in o] for o in outs]


def check_entry(e, got):
    kind, c = e["kind"], e["c"]
    what = f"kind {kind} {c['id']}"
    if kind == 0:
        return C.check_pack(c, e["data"], e["dt"], got[0], what)
    if kind in (1, 4):
        return C.check_sum(got[0], C.reduce_model(c, e["data"]), what)
    if kind == 2:
        return C.check_sum(got[0], C.rows2_model(c, e["data"]), what)
    if kind == 3:
        return C.check_convpack(c, e["data"], got[0], got[1], what)
    return C.check_gather(c, e["data"], got[0].view(torch.int32).view(c["rows"], c["fe"]), what)


def test_job_table_every_launch_shape_bounded_exact_and_equal_to_the_direct_forms(lib):
    entries = table_inputs()
    before = [bits(e["src"].buf) for e in entries]
    runs = [run_table(lib, entries, how, arg) for how, arg in LAUNCHES]
    for e, b in zip(entries, before):
        assert torch.equal(bits(e["src"].buf), b), f"kind {e['kind']} {e['c']['id']}: a launch wrote to its input"
    rows, first = runs[0]
    assert {C.job_branch(r) for r in rows} == {b for b in C.LAYOUT_BRANCHES if b.startswith("run_jobs_k")}
    for (how, arg), (_, outs) in zip(LAUNCHES[1:], runs[1:]):
        for e, a, b in zip(entries, first, outs):
            for x, y in zip(a, b):
                assert torch.equal(bits(x), bits(y)), f"kind {e['kind']} {e['c']['id']}: {how} {arg} differs from one workgroup per job"
    worst = {}
    for e, r, got in zip(entries, rows, first):
        k = C.job_branch(r)
        worst[k] = max(worst.get(k, 0.0), check_entry(e, got))
    report("run_jobs", "mixed table", worst)
    # the same f32 operations in the same order as the direct entry points (a preloaded output may meet a fused multiply-add)
    for e, got in zip(entries, first):
        kind, c = e["kind"], e["c"]
        if kind == 0:
            ref = direct_pack(lib, c, e["dt"], e["src"])
        elif kind in (1, 4) and not c["acc"]:
            ref = direct_reduce(lib, c, e["src"], None)
        elif kind == 5:
            ref = direct_gather(lib, c, e).view(torch.float32).reshape(-1)
        else:
            continue
        assert torch.equal(bits(got[0]), bits(ref)), f"kind {kind} {c['id']}: the job differs from its direct entry point"


# ---- refusals: the error, the entry point's name, and nothing written -------------------------------------------------------------------------

def test_refusals_name_the_entry_point_and_write_nothing(lib):
    x, xb = flat(torch.randn(4096)), flat(torch.randn(4096), BF)
    o1, o2, o3 = flat_out(4096), flat_out(4096), flat_out(4096, dtype=BF)
    ints = torch.zeros(64, dtype=torch.int32, device="cuda")
    plan = torch.zeros(8, dtype=torch.int64, device="cuda")

    def refused(name, word, *args):
        with pytest.raises(ValueError) as err:
            lib.call(name, *args)
        torch.cuda.synchronize()
        msg = lib.query("rbvae_last_error").decode()
        assert msg.startswith(word + ":") and msg in str(err.value), (name, msg)
        untouched(o1, o2, o3)

    sk = lambda *a: ("skinny_linear", *a)
    refused("rbvae_skinny_linear", *sk(F32_T, x.view, x.view, None, o1.view, 4, 4, 24, 32, 32, 4))                 # K % 16
    refused("rbvae_skinny_linear", *sk(BF16_T, xb.view, xb.view, None, o1.view, 4, 4, 48, 64, 64, 4))              # K % 32
    refused("rbvae_skinny_linear", *sk(F32_T, x.view.data_ptr() + 4, x.view, None, o1.view, 4, 4, 32, 32, 32, 4))  # misaligned A
    refused("rbvae_skinny_linear", *sk(F32_T, x.view, x.view.data_ptr() + 8, None, o1.view, 4, 4, 32, 32, 32, 4))  # misaligned B
    refused("rbvae_skinny_linear", *sk(F32_T, x.view, x.view, None, o1.view, 4, 4, 32, 30, 32, 4))                 # lda * 4 % 16
    refused("rbvae_skinny_linear", *sk(F32_T, x.view, x.view, None, o1.view, 4, 4, 32, 16, 32, 4))                 # lda < K
    refused("rbvae_skinny_linear", *sk(F32_T, x.view, x.view, None, o1.view, 4, 4, 32, 32, 32, 3))                 # ldo < Nc
    refused("rbvae_skinny_linear", *sk(7, x.view, x.view, None, o1.view, 4, 4, 32, 32, 32, 4))                     # dtype
    refused("rbvae_skinny_linear_parts", *sk(F32_T, x.view, x.view, None, o1.view, 4, 4, 48, 48, 48, 4, 2))        # K % (ksplit * 16)
    refused("rbvae_skinny_linear_parts", *sk(BF16_T, xb.view, xb.view, None, o1.view, 4, 4, 96, 96, 96, 4, 2))     # K % (ksplit * 32)
    refused("rbvae_skinny_linear_parts", *sk(F32_T, x.view, x.view, None, o1.view, 4, 4, 32, 32, 32, 4, 0))        # ksplit
    refused("rbvae_gather_frames", "gather_frames", x.view, 4, plan, 2, 1, None, 6, o1.view)                        # frame_elems % 4
    refused("rbvae_gather_frames", "gather_frames", x.view.data_ptr() + 4, 4, plan, 2, 1, None, 8, o1.view)         # misaligned table
    refused("rbvae_gather_frames", "gather_frames", x.view, 4, plan, 2, 1, None, 8, o1.view.data_ptr() + 8)         # misaligned out
    refused("rbvae_gather_frames", "gather_frames", x.view, 0, plan, 2, 1, None, 8, o1.view)                        # no table rows
    vote = lambda L, keys: ("state_vote", x.view, ints, 8, L, 2, keys, o2.view, o1.view.data_ptr() + 64)
    refused("rbvae_state_vote", *vote(0, o1.view))
    refused("rbvae_state_vote", *vote(129, o1.view))
    refused("rbvae_state_vote", *vote(16, o1.view.data_ptr() + 4))                                                  # misaligned keys
    refused("rbvae_pack3", "pack3", 7, x.view, o1.view, 2, 3, 4, 12, 4, 1)
    refused("rbvae_pack3", "pack3", F32_T, x.view, o1.view, 0, 3, 4, 12, 4, 1)
    refused("rbvae_cast_pad", "cast_pad", 7, x.view, o1.view, 2, 8, 16)
    refused("rbvae_cast_pad", "cast_pad", BF16_T, x.view, o3.view, 2, 16, 8)                                        # Lpad < L
    refused("rbvae_colsum", "colsum", 7, x.view, 4, 8, 8, o1.view, o2.view, 1.0, 0)
    refused("rbvae_colsum", "colsum", F32_T, x.view, 4, 8, 7, o1.view, o2.view, 1.0, 0)                             # ld < C
    refused("rbvae_colsum_partial", "colsum_partial", 7, x.view, 4, 8, 8, o2.view)
    refused("rbvae_colsum_partial", "colsum_partial", BF16_T, xb.view, 4, 8, 7, o2.view)                            # ld < C
    refused("rbvae_permute_reduce", "permute_reduce", x.view, 0, 24, o1.view, 2, 3, 4, 12, 4, 1, 1.0, 0)
    refused("rbvae_reduce_rows", "reduce_rows", x.view, 0, 8, o1.view, 1.0, 0)


# ---- coverage (runs last) ---------------------------------------------------------------------------------------------------------------

def test_every_entry_point_of_the_docstring_was_called():
    want = set(re.findall(r"rbvae_\w+", __doc__)) - {"rbvae_last_error"}
    assert len(want) == 14, sorted(want)
    assert C.covered_branches() == set(C.LAYOUT_BRANCHES)
    if CALLED:                                                  # empty: this test was selected alone, nothing to account for
        assert want <= CALLED, f"never called: {sorted(want - CALLED)}"
