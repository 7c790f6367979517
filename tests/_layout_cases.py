"""References, error model, f32 emulations, dispatch restatements and case tables for the layout, reduce and job kernel bounds
tests: the "layout and small dense helpers" of csrc/layout.hip (pack3_k, permute_reduce_k, cast_pad_k, colsum_partial_k,
colsum_partial_vec_k, colsum_final_k, skinny_linear_k, gather_frames_k), the non-Adam branches of run_jobs_k (kinds 0-5,
csrc/jobs.hip) and the state vote of csrc/eval.hip.  Plain torch / numpy on the CPU: importing this module needs no GPU.

Error model (u = 2^-24; derived, not tuned)
    A sum of f32 terms v, scaled and optionally accumulated:  out = prev + scale * sum v.  Every term passes through at most h
    f32 additions (the summation height of the branch, restated below from its code), the scaling is one rounding and the
    accumulation one more:
        |out - ref| <= |scale| h u sum|v| + u |scale sum v| (+ u |prev + scale sum v|) + TINY
    Heights (additions any one input passes through; a chain that starts from 0.f counts its first addition too, which only
    loosens the height by one):
        permute_reduce_k, kinds 1 (generic and inner) and 4      nslab       one chain in slab order, whatever the unrolling
        colsum_partial_k                 ceil(rows of the block / rl) + rl   rl = 256 / min(C, 256) row lanes, then their chain
        colsum_partial_vec_k             rows of the block                   one chain in row order (4-row groups add in order)
        colsum_final_k (reduce_rows)     ceil(nblk / 4) + 3                  4 row lanes, then ((r0 + r1) + r2) + r3
        kind 2, wave path                ceil(nslab / 64) + 6                lane-strided chain, 6 wave_sum levels
        kind 2, wide path                ceil(nslab / 256) + 8               thread-strided chain, 8 tree levels
    rbvae_colsum is the partial height plus the final height.  The bf16 operands are exact in f32.
    skinny_linear_k: tests/_bounds.check with c_acc(K of the part) and S = sum |a b| (+ |bias|), as the GEMM tests do.
    Input condition (asserted on the CPU): summands have |v| in [0.5, 2] with random sign, and for every output of every sum
    case  min|term| |scale| >= 8 bound,  so a dropped, doubled or misplaced term is at least 8 bounds away.

Exact operations
    pack3 / kind 0 / kind 3 / cast_pad: the f32 value itself or torch's round-to-nearest-even .to(bfloat16), bit for bit,
    through the restated index map; a NaN input comes out as some NaN.  gather / kind 5: 32-bit patterns unchanged.
    state_vote: integers.  What a call does not declare stays sentinel (emulations write into sentinel-filled buffers too, so
    the same check sees a stray or missing store on the CPU and on the device).

The winner's KEY of the state vote never leaves the device (out holds its count and the state's frame count only), so the
tie rule -- smallest key in element-0-first order -- is checked on the emulation alone (`winners`), against np.unique."""
import struct

import numpy as np
import torch

import _bounds as B
from _bounds import TINY, U32
from _loss_cases import BF16_T, CPK_CIB, CPK_MAXROW, F32_T, TDT, cdiv, conv_pack_path, gen_of, job_kernel, perm_strides, tile_shape, wave_sum32
from _lstm_cases import _exact, _worst

U = U32
D, F, BF = torch.float64, torch.float32, torch.bfloat16
DTN = {F32_T: "f32", BF16_T: "bf16"}
ES = {F32_T: 4, BF16_T: 2}
CRD_CI = 256


# ---- buffers of sentinels on the CPU ---------------------------------------------------------------------------------------

def sentinel(shape, dtype=F):
    ib, pat = B.SENTINEL[dtype]
    return torch.full(tuple(shape) if not isinstance(shape, int) else (shape,), pat, dtype=ib).view(dtype)


def is_sentinel(t):
    ib, pat = B.SENTINEL[t.dtype]
    return t.contiguous().view(ib) == pat


def check_written(got, written, what):
    """Exactly the elements of `written` left the sentinel."""
    s = is_sentinel(got).reshape(-1)
    w = written.reshape(-1)
    assert s.numel() == w.numel(), f"{what}: output of {s.numel()} elements, declared {w.numel()}"
    stray = (~s & ~w).nonzero()
    assert stray.numel() == 0, f"{what}: {stray.numel()} undeclared elements were written, first at {int(stray[0])}"
    miss = (s & w).nonzero()
    assert miss.numel() == 0, f"{what}: {miss.numel()} declared elements were never written, first at {int(miss[0])}"


def signed(gen, *shape, dtype=F):
    """|v| in [0.5, 2] with random sign, representable in dtype; returned as f32."""
    mag = 0.5 + 1.5 * torch.rand(*shape, generator=gen)
    sgn = torch.randint(0, 2, shape, generator=gen).to(F) * 2 - 1
    return (mag * sgn).to(dtype).to(F)


def from_bits(bits):
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(F)


# +-0, subnormals, values that round up into the next binade in bf16, ties to even / to odd, overflow to inf, +-inf, NaNs
SPECIALS = from_bits([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x3F7FFFFF, 0xBFFFFFFF, 0x3F808000, 0x3F818000,
                      0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFD12345])


def with_specials(gen, n):
    x = torch.randn(n, generator=gen)
    k = min(n, SPECIALS.numel())
    x[:k] = SPECIALS[:k]
    return x


def check_exact(got, want, src, what, dims=("element",)):
    """got == want bit for bit except where the f32 source is NaN: there any NaN."""
    nan = torch.isnan(src).reshape(got.shape)
    assert bool(torch.isnan(got.float()[nan]).all()), f"{what}: a NaN input did not come out as NaN"
    z = torch.zeros((), dtype=got.dtype)
    return _exact(torch.where(nan, z, got), torch.where(nan, z, want), what, dims)


def store(x, dt, defect=None):
    """The storage rounding of Elem<T>::store."""
    if dt == BF16_T and defect == "bf16_truncates":
        return (x.contiguous().view(torch.int32) >> 16).to(torch.int16).view(BF)
    return x.to(TDT[dt])


def idx3(dims, strides):
    """Strided-side offset of every logical element, in the contiguous side's order."""
    i = torch.meshgrid(*[torch.arange(d) for d in dims], indexing="ij")
    return (i[0] * strides[0] + i[1] * strides[1] + i[2] * strides[2]).reshape(-1)


def numel(dims):
    return dims[0] * dims[1] * dims[2]


# ---- the sum model ------------------------------------------------------------------------------------------------------------

def sum_model(terms, h, scale=1.0, prev=None):
    """terms [k][n] (f32 values) -> dict(ref, bnd, minterm) of prev + scale * sum_k terms (module docstring)."""
    t = terms.to(D)
    s, sabs = t.sum(0), t.abs().sum(0)
    ref = scale * s
    bnd = abs(scale) * h * U * sabs + U * ref.abs() + TINY
    if prev is not None:
        ref = prev.to(D) + ref
        bnd = bnd + U * ref.abs()
    return dict(ref=ref, bnd=bnd, minterm=t.abs().min(0).values * abs(scale), h=h)


def check_sum(got, model, what, dims=("output",)):
    return _worst((got.to(D).reshape(model["ref"].shape) - model["ref"]).abs(), model["bnd"], what, dims)


def chain32(x):
    """acc = 0; acc += x[k] over the first axis, in order, in f32."""
    acc = torch.zeros(x.shape[1:], dtype=F)
    for k in range(x.shape[0]):
        acc = acc + x[k]
    return acc


def finish32(a, scale, prev, defect=None):
    a = a * torch.tensor(float(scale), dtype=F)
    return prev + a if prev is not None and defect != "accumulate_ignored" else a


# ---- the job table: rows, workgroups, branches (restating engine.JobList and csrc/jobs.hip) --------------------------------------

def job_row(kind, src, dst, dims, strides=(0, 0, 0), nslab=1, slab=0, dtype=0, acc=0, scale=1.0, dst2=0):
    """One 16 x int64 row as engine.JobList builds it (add / add_conv_pack / add_conv_reduce / the gather row)."""
    bits = struct.unpack("<I", struct.pack("<f", float(scale)))[0]
    if kind in (0, 1, 2):
        fast = 2
        for ax in (2, 1, 0):
            if strides[ax] == 1 and dims[ax] > 1:
                fast = ax
                break
        inner = int(kind in (0, 1) and fast == 1 and dims[2] <= 16 and dims[1] >= 64)
        return [kind, src, dst, *dims, *strides, nslab, slab, dtype, int(acc), bits | (fast << 32), inner, 0]
    if kind == 3:
        return [3, src, dst, *dims, 0, 0, 0, 1, 0, dtype, 0, 0, 0, dst2]
    if kind == 4:
        return [4, src, dst, *dims, 0, 0, 0, nslab, slab, 0, int(acc), bits, 0, 0]
    assert kind == 5                       # dims = (rows, batches, float4 per row), strides = (plan, counter or 0, table rows)
    return [5, src, dst, *dims, *strides, 0, 0, 0, 0, 0, 0, 0]


def conv_pack_pieces(Co, Ci, kk, dt):
    """(vec_ok, cib, pieces) of conv_pack_rows."""
    nv = 16 // ES[dt]
    cib = min((CPK_MAXROW // kk) // nv * nv, Ci)
    if cib > CPK_CIB and Ci % CPK_CIB == 0:
        cib = CPK_CIB
    vec = Ci % nv == 0 and Co % nv == 0 and (cib * kk) % 4 == 0 and (Ci * kk) % 4 == 0
    assert (("vec" if vec else "elem"), cdiv(Ci, cib)) == conv_pack_path(dict(dims=(Co, Ci, kk), dtype=dt))
    return vec, cib, cdiv(Ci, cib)


def update_job_of(r):
    """The _loss_cases.job description of a fused-update row (kind 3 with a context, 6, 7), read back from its fields."""
    kind, dims = r[0], tuple(r[3:6])
    if kind != 6:
        return dict(id="row", kind=kind, dims=dims, dtype=r[11], copies=())
    copies = [(r[11] & 255, tuple(r[6:9]))] + ([((r[11] >> 8) & 255, (r[9], r[10], r[12]))] if r[15] else [])
    return dict(id="row", kind=6, dims=dims, dtype=0, copies=tuple(copies))


def job_blocks_of(r):
    """Workgroups a row can use: job_blocks_of of csrc/jobs.hip, every kind (kind 6 from _loss_cases.tile_shape)."""
    kind, d0, d1, d2 = r[0], r[3], r[4], r[5]
    n = d0 * d1 * d2
    if kind == 3:
        nco = 16 // ES[r[11] & 255]
        return cdiv(d0, nco) * conv_pack_pieces(d0, d1, d2, r[11] & 255)[2]
    if kind == 4:
        return d0 * cdiv(d1, CRD_CI)
    if kind == 5:
        return d0
    if kind == 6:
        ts = tile_shape(update_job_of(r))
        return cdiv(n, 256) if ts is None else cdiv(d0, ts[0]) * cdiv(d1, ts[1]) * cdiv(d2, ts[2])
    if kind == 7:
        return cdiv(n, 256)
    if kind == 2:
        return cdiv(n, 4)
    if r[14]:
        return cdiv(d0 * d1, 256)
    return cdiv(n, 256)


def block_map(rows, cap):
    """rbvae_job_block_map: (job, workgroup within the job, workgroups of the job, 0) per workgroup, at most cap per job."""
    out = []
    for j, r in enumerate(rows):
        nb = min(max(job_blocks_of(r), 1), cap)
        out += [[j, b, nb, 0] for b in range(nb)]
    return out


def job_branch(r):
    """The branch of run_jobs_k a row takes, in the kernel's order of tests."""
    kind, d0, d1, d2 = r[0], r[3], r[4], r[5]
    n = d0 * d1 * d2
    if kind in (6, 7) or (kind == 3 and r[14]):
        return job_kernel(update_job_of(r))                 # the fused-update branches, named as in _loss_cases.JOB_BRANCHES
    if kind == 3:
        vec, _, pieces = conv_pack_pieces(d0, d1, d2, r[11])
        return f"run_jobs_k[3,{'vec' if vec else 'elem'},{DTN[r[11]]}{',split' if pieces > 1 else ''}]"
    if kind == 4:
        na = cdiv(d2 * (min(d1, CRD_CI) // 4), 256)
        return f"run_jobs_k[4,na{na}{',ncb' if d1 > CRD_CI else ''}]"
    if kind == 5:
        return "run_jobs_k[5]"
    if kind == 2:
        wide = r[9] >= 1024 and n % 4 == 0 and r[10] % 4 == 0 and r[1] % 16 == 0
        return "run_jobs_k[2,wide]" if wide else "run_jobs_k[2,wave]"
    if r[14]:
        return f"run_jobs_k[{kind},inner{',4slabs' if kind == 1 and d2 <= 9 and r[9] >= 4 else ''}]"
    return f"run_jobs_k[{kind},fast{r[13] >> 32}]"


# ---- pack3 / kind 0 ---------------------------------------------------------------------------------------------------------------

def pk(id, dims, order=None, strides=None, job=True):
    return dict(id=id, dims=dims, strides=tuple(strides or perm_strides(dims, order)), job=job)


PACK_CASES = [
    pk("conv5x7x9", (5, 7, 9), (0, 2, 1)),                    # [co][ci][kk] -> [co][t][ci]: fast = 1, rows too short for `inner`
    pk("fast2", (4, 6, 5), (1, 0, 2)), pk("fast0", (6, 5, 3), (2, 1, 0)),
    pk("fast2-600", (10, 12, 5), (1, 0, 2)),                  # 3 workgroups of a job
    pk("gaps", (4, 6, 5), strides=(52, 8, 1)),                # rows of 5 in a pitch of 8, 4 more elements between planes
    pk("inner-kk1", (5, 64, 1), (0, 2, 1)), pk("inner-kk4", (2, 65, 4), (0, 2, 1)), pk("inner-kk9", (5, 64, 9), (0, 2, 1)),
    pk("inner-kk16", (2, 70, 16), (0, 2, 1)),
    pk("grid-stride", (130, 97, 84), (0, 2, 1), job=False),   # 1 059 240 > 256 x 4096 elements: the direct kernel's loop iterates
]


def pack_data(c):
    return with_specials(gen_of(1, *c["dims"]), numel(c["dims"]))


def pack_branch(c, dt):
    return f"pack3_k<{DTN[dt]}>" + ("[grid-stride]" if numel(c["dims"]) > 256 * 4096 else "")


def pack_span(c):
    return int(idx3(c["dims"], c["strides"]).max()) + 1


def emu_pack(c, x, dt, defect=None):
    s = c["strides"]
    if defect == "pack_strides_swapped":
        s = (s[0], s[2], s[1])
    idx = idx3(c["dims"], s)
    out = sentinel(max(pack_span(c), int(idx.max()) + 1), TDT[dt])
    out[idx] = store(x, dt, defect)
    return out


def check_pack(c, x, dt, got, what):
    idx = idx3(c["dims"], c["strides"])
    assert idx.unique().numel() == idx.numel()
    written = torch.zeros(pack_span(c), dtype=torch.bool)
    written[idx] = True
    assert got.dtype == TDT[dt]
    check_written(got, written, what)
    return check_exact(got[idx], x.to(TDT[dt]), x, what, ("source element",))


# ---- permute_reduce / kind 1 ---------------------------------------------------------------------------------------------------------

def pr(id, dims, order, nslab, gap=0, scale=1.0, acc=0, job=True):
    return dict(id=id, dims=dims, strides=perm_strides(dims, order), nslab=nslab, slab=numel(dims) + gap, scale=scale, acc=acc, job=job)


PERMUTE_CASES = (
    [pr(f"ns{ns}", (3, 5, 7), (2, 0, 1), ns, scale=(1.0, 0.5, -1.25)[i % 3], acc=i % 2) for i, ns in enumerate((1, 2, 3, 4, 5, 7, 16, 17, 21))]
    + [pr("fast2-2wg", (9, 10, 5), (1, 0, 2), 3), pr("fast0", (6, 5, 3), (2, 1, 0), 5, scale=0.5, acc=1),
       pr("gap", (3, 5, 7), (0, 2, 1), 6, gap=11, scale=-1.25),
       pr("inner-kk9-ns3", (5, 64, 9), (0, 2, 1), 3), pr("inner-kk9-ns4", (2, 64, 9), (0, 2, 1), 4, scale=0.5),
       pr("inner-kk9-ns7", (2, 66, 9), (0, 2, 1), 7, gap=5, acc=1), pr("inner-kk16-ns5", (2, 64, 16), (0, 2, 1), 5, scale=-1.25, acc=1),
       pr("inner-kk4", (3, 70, 4), (0, 2, 1), 9, scale=0.5)])


def reduce_data(c, key=2):
    """(slabs [nslab * slab] with NaN in the gap between slabs, prev [n] or None)."""
    g = gen_of(key, *c["dims"], c["nslab"])
    n = numel(c["dims"])
    src = torch.full((c["nslab"], c["slab"]), float("nan"))
    src[:, :n] = signed(g, c["nslab"], n)
    return src.reshape(-1), (signed(g, n) if c["acc"] else None)


def reduce_terms(c, src):
    """[nslab][n] in the contiguous side's order."""
    return src.view(c["nslab"], c["slab"])[:, idx3(c["dims"], c["strides"])]


def reduce_model(c, data):
    return sum_model(reduce_terms(c, data[0]), c["nslab"], c["scale"], data[1])


def emu_reduce(c, data, defect=None):
    t = reduce_terms(c, data[0])
    if defect == "drop_last_slab":
        t = t[:-1]
    return finish32(chain32(t), c["scale"], data[1], defect)


# ---- cast_pad ---------------------------------------------------------------------------------------------------------------------------

CASTPAD_CASES = [dict(id=f"{r}x{L}->{Lp}-{DTN[dt]}", rows=r, L=L, Lpad=Lp, dt=dt)
                 for r, L, Lp in ((3, 25, 64), (4, 32, 32), (5, 100, 104)) for dt in (F32_T, BF16_T)]


def castpad_data(c):
    return with_specials(gen_of(3, c["rows"], c["L"]), c["rows"] * c["L"]).view(c["rows"], c["L"])


def emu_castpad(c, x, defect=None):
    r, L, Lp = c["rows"], c["L"], c["Lpad"]
    out = sentinel((r, Lp), TDT[c["dt"]])
    if defect == "cast_pad_no_select":                       # in[r * L + c] for every c < Lpad
        flat = torch.cat([x.reshape(-1), torch.ones(Lp)])
        i = torch.arange(r)[:, None] * L + torch.arange(Lp)[None]
        out[:] = store(flat[i], c["dt"])
        return out
    out[:, :L] = store(x, c["dt"], defect)
    out[:, L:] = 0
    return out


def check_castpad(c, x, got, what):
    check_written(got, torch.ones(c["rows"], c["Lpad"], dtype=torch.bool), what)
    want = torch.zeros(c["rows"], c["Lpad"], dtype=TDT[c["dt"]])
    want[:, :c["L"]] = x.to(TDT[c["dt"]])
    src = torch.zeros(c["rows"], c["Lpad"])
    src[:, :c["L"]] = x
    return check_exact(got, want, src, what, ("row", "column"))       # bit for bit: the padding is +0


# ---- column sums ----------------------------------------------------------------------------------------------------------------------------

def colsum_rpb(P):
    return max(16, ((cdiv(P, 256) + 15) // 16) * 16)


def colsum_nblk(P):
    return cdiv(P, colsum_rpb(P))


def colsum_ws_floats(P, C):
    return colsum_nblk(P) * C


def colsum_vec(c):
    """launch_colsum_partial's test (X and ws are 16-byte aligned up to the case's element offsets)."""
    ec = 16 // ES[c["dt"]]
    return (c["C"] >= 2048 and c["C"] % ec == 0 and c["ld"] % ec == 0 and (c["xoff"] * ES[c["dt"]]) % 16 == 0
            and (c["wsoff"] * 4) % 16 == 0)


def colsum_branch(c):
    return f"colsum_partial_{'vec_' if colsum_vec(c) else ''}k<{DTN[c['dt']]}>"


def colsum_rl(c):
    return 256 // min(c["C"], 256)


def partial_height(c, rows):
    return rows if colsum_vec(c) else cdiv(rows, colsum_rl(c)) + colsum_rl(c)


def final_height(nblk):
    return cdiv(nblk, 4) + 3


def cs(id, dt, P, C, ld=None, scale=1.0, acc=0, xoff=0, wsoff=0):
    return dict(id=f"{id}-{DTN[dt]}", dt=dt, P=P, C=C, ld=ld or C, scale=scale, acc=acc, xoff=xoff, wsoff=wsoff)


COLSUM_CASES = (
    [cs(f"C{C}", (F32_T, BF16_T)[i % 2], 37, C, ld=C + (0, 8, 0)[i % 3], scale=(1.0, 0.5, -1.25)[i % 3], acc=i % 2)
     for i, C in enumerate((1, 3, 25, 100, 256, 300))]
    + [cs(f"P{P}", (BF16_T, F32_T)[i % 2], P, 25, ld=32, scale=(0.5, 1.0)[i % 2], acc=(i + 1) % 2) for i, P in enumerate((1, 15, 16, 17, 19))]
    + [cs("P4097", F32_T, 4097, 260, ld=264, scale=-1.25, acc=1),                               # rpb = 32, 129 partial rows
       cs("vec-P19", F32_T, 19, 2048), cs("vec-P19", BF16_T, 19, 2048, ld=2056, scale=0.5),   # a 3-row tail
       cs("vec-P38", F32_T, 38, 2048, ld=2052, acc=1), cs("vec-P38", BF16_T, 38, 2048),       # 4-row loop, 2-row tail in block 2
       cs("vec-C2056", F32_T, 21, 2056, scale=-1.25), cs("vec-C2056", BF16_T, 21, 2056, ld=2064, acc=1),   # ragged last group
       cs("fall-C2052", BF16_T, 19, 2052, ld=2056), cs("fall-ld", F32_T, 19, 2048, ld=2050),
       cs("fall-xoff", F32_T, 19, 2048, ld=2052, xoff=1), cs("fall-xoff", BF16_T, 19, 2048, ld=2056, xoff=1),
       cs("fall-wsoff", F32_T, 19, 2048, wsoff=1)])
REDUCE_ROWS_CASES = [dict(id=f"{r}x{C}", rows=r, C=C, scale=(1.0, 0.5, -1.25)[(i + k) % 3], acc=(i + k) % 2)
                     for i, r in enumerate((1, 3, 4, 5, 1000)) for k, C in enumerate((1, 63, 64, 65, 130))]


def colsum_data(c):
    """(X [P][C] in f32, already rounded to the storage type; prev [C] or None)."""
    g = gen_of(4, c["P"], c["C"], c["dt"])
    return signed(g, c["P"], c["C"], dtype=TDT[c["dt"]]), (signed(g, c["C"]) if c["acc"] else None)


def _blocks(c, X):
    rpb = colsum_rpb(c["P"])
    return [X[r0:min(c["P"], r0 + rpb)] for r0 in range(0, c["P"], rpb)]


def partial_model(c, X):
    ms = [sum_model(b, partial_height(c, b.shape[0])) for b in _blocks(c, X)]
    return {k: torch.stack([m[k] for m in ms]) for k in ("ref", "bnd", "minterm")}


def colsum_model(c, data):
    X, prev = data
    h = max(partial_height(c, b.shape[0]) for b in _blocks(c, X)) + final_height(colsum_nblk(c["P"]))
    return sum_model(X, h, c["scale"], prev)


def emu_colsum_partial(c, X, defect=None):
    """ws [nblk][C] (sentinel where a defect leaves it unwritten)."""
    blocks, rpb, C = _blocks(c, X), colsum_rpb(c["P"]), c["C"]
    ws = sentinel((len(blocks), C))
    vec, rl = colsum_vec(c), colsum_rl(c)
    for b, rows in enumerate(blocks):
        n = rows.shape[0]
        if defect == "colsum_drops_short_block" and n < rpb:
            continue
        if vec:
            if defect == "vec_drops_row_tail":
                rows = rows[:n // 4 * 4]
            ws[b] = chain32(rows)
            if defect == "vec_skips_ragged_group":
                per = 256 * (16 // ES[c["dt"]])
                ws[b, C // per * per:] = sentinel(C - C // per * per)
        else:
            steps = cdiv(n, rl)
            p = torch.zeros(steps * rl, C)
            p[:n] = rows
            ws[b] = chain32(chain32(p.view(steps, rl, C)))           # each lane's chain, then the lanes in order
    return ws


def emu_final(ws, scale, prev, defect=None):
    nblk, C = ws.shape
    if defect == "final_drops_row_tail":
        ws = ws[:nblk // 4 * 4]
        nblk = ws.shape[0]
    steps = cdiv(nblk, 4)
    p = torch.zeros(max(steps, 1) * 4, C)
    p[:nblk] = ws
    r = chain32(p.view(-1, 4, C))
    return finish32(((r[0] + r[1]) + r[2]) + r[3], scale, prev, defect)


def emu_colsum(c, data, defect=None):
    ws = emu_colsum_partial(c, data[0], defect)
    if defect == "colsum_drops_short_block":
        ws = ws[~is_sentinel(ws).all(1)]
    return emu_final(ws, c["scale"], data[1], defect)


def reduce_rows_data(c):
    g = gen_of(5, c["rows"], c["C"])
    return signed(g, c["rows"], c["C"]), (signed(g, c["C"]) if c["acc"] else None)


def reduce_rows_model(c, data):
    return sum_model(data[0], final_height(c["rows"]), c["scale"], data[1])


# ---- kind 2: rows of partial sums ------------------------------------------------------------------------------------------------------

def r2(nslab, n, slab=None, soff=0, scale=1.0, acc=0):
    slab = slab or n
    return dict(id=f"ns{nslab}-n{n}" + (f"-slab{slab}" if slab != n else "") + ("-off" if soff else ""), nslab=nslab, n=n, slab=slab,
                soff=soff, scale=scale, acc=acc)


ROWS2_CASES = (
    [r2(ns, (1, 3, 5)[i % 3], slab=8, scale=(1.0, 0.5, -1.25)[i % 3], acc=i % 2) for i, ns in enumerate((1, 63, 64, 65, 448, 449, 513, 1023))]
    + [r2(ns, (4, 8, 64)[i % 3], slab=(4, 12, 64)[i % 3], scale=(0.5, -1.25, 1.0)[i % 3], acc=(i + 1) % 2)
       for i, ns in enumerate((1024, 1025, 1792, 1793, 2049))]
    + [r2(1024, 6, slab=8), r2(1024, 4, slab=5, scale=0.5), r2(1024, 8, soff=1, acc=1)])      # three ways back to the wave path


def rows2_row(c, src=0, dst=0):
    return job_row(2, src + 4 * c["soff"], dst, (1, 1, c["n"]), (0, 0, 1), nslab=c["nslab"], slab=c["slab"], acc=c["acc"], scale=c["scale"])


def rows2_wide(c):
    return job_branch(rows2_row(c)) == "run_jobs_k[2,wide]"


def rows2_data(c):
    g = gen_of(6, c["nslab"], c["n"], c["slab"])
    src = torch.full((c["nslab"], c["slab"]), float("nan"))
    src[:, :c["n"]] = signed(g, c["nslab"], c["n"])
    return src, (signed(g, c["n"]) if c["acc"] else None)


def rows2_height(c):
    return cdiv(c["nslab"], 256) + 8 if rows2_wide(c) else cdiv(c["nslab"], 64) + 6


def rows2_model(c, data):
    return sum_model(data[0][:, :c["n"]], rows2_height(c), c["scale"], data[1])


def emu_rows2(c, data, defect=None):
    x, ns, n = data[0][:, :c["n"]], c["nslab"], c["n"]
    lanes = 256 if rows2_wide(c) else 64
    if defect == "wide_drops_tail" and rows2_wide(c):
        ns = ns // 2048 * 2048
        x = x[:ns]
    steps = max(cdiv(ns, lanes), 1)
    p = torch.zeros(steps * lanes, n)
    p[:ns] = x
    a = chain32(p.view(steps, lanes, n))                        # [lanes][n]
    if rows2_wide(c):
        s = 128
        while s:
            a = a[:s] + a[s:2 * s]
            s //= 2
        t = a[0]
    else:
        t = wave_sum32(a.t().contiguous())
    return finish32(t, c["scale"], data[1], defect)


# ---- kind 3 without an optimiser context -----------------------------------------------------------------------------------------------

def cp(Co, Ci, kk, dt):
    return dict(id=f"{Co}x{Ci}x{kk}-{DTN[dt]}", dims=(Co, Ci, kk), dt=dt)


CONVPACK_CASES = [cp(8, 8, 1, F32_T), cp(8, 16, 4, BF16_T), cp(8, 8, 9, F32_T), cp(8, 16, 16, BF16_T), cp(8, 16, 9, BF16_T),
                  cp(5, 6, 9, F32_T), cp(5, 6, 4, BF16_T), cp(4, 128, 9, F32_T), cp(8, 128, 4, BF16_T), cp(8, 328, 9, BF16_T),
                  cp(4, 328, 9, F32_T), cp(8, 160, 16, BF16_T)]


def convpack_data(c):
    return with_specials(gen_of(7, *c["dims"]), numel(c["dims"])).view(c["dims"])


def emu_convpack(c, x, defect=None):
    """(wf [co][t][ci], wd [ci][t][co]) written piece by piece."""
    Co, Ci, kk = c["dims"]
    _, cib, pieces = conv_pack_pieces(Co, Ci, kk, c["dt"])
    wf, wd = sentinel((Co, kk, Ci), TDT[c["dt"]]), sentinel((Ci, kk, Co), TDT[c["dt"]])
    v = store(x, c["dt"], defect)
    for p in range(pieces):
        ci0 = p * cib
        cn = min(cib, Ci - ci0)
        o = 0 if defect == "pack_loses_ci0" else ci0
        wf[:, :, o:o + cn] = v[:, ci0:ci0 + cn].permute(0, 2, 1)
        wd[o:o + cn] = v[:, ci0:ci0 + cn].permute(1, 2, 0)
    if defect == "dst2_in_dst_order":
        wd = wf.clone().view(Ci, kk, Co)
    return wf, wd


def check_convpack(c, x, wf, wd, what):
    Co, Ci, kk = c["dims"]
    t = TDT[c["dt"]]
    for name, got, want, src in (("dst", wf, x.permute(0, 2, 1), x.permute(0, 2, 1)), ("dst2", wd, x.permute(1, 2, 0), x.permute(1, 2, 0))):
        got = got.reshape(want.shape)
        check_written(got, torch.ones(want.shape, dtype=torch.bool), f"{what} {name}")
        check_exact(got, want.to(t).contiguous(), src.contiguous(), f"{what} {name}", ("row", "tap", "channel"))
    return 0.0


# ---- kind 4: weight-gradient slabs -------------------------------------------------------------------------------------------------------

def cr(Co, Ci, kk, nslab, scale=1.0, acc=0):
    return dict(id=f"{Co}x{Ci}x{kk}-ns{nslab}", dims=(Co, Ci, kk), strides=(kk * Ci, 1, Ci), nslab=nslab, slab=Co * kk * Ci, scale=scale, acc=acc)


CONVRED_CASES = (
    [cr(3, 64, 9, ns, scale=(1.0, 0.5, -1.25)[i % 3], acc=i % 2) for i, ns in enumerate((1, 2, 7, 8, 9, 17))]
    + [cr(2, 256, kk, ns, scale=(0.5, 1.0, -1.25)[ns % 3], acc=(ns + kk) % 2) for kk in (9, 16) for ns in (1, 2, 3)]
    + [cr(2, 260, 9, 3, scale=0.5), cr(2, 520, 4, 2, acc=1), cr(2, 260, 1, 9, scale=-1.25)])


def emu_convred(c, data, defect=None):
    Co, Ci, kk = c["dims"]
    t = reduce_terms(c, data[0]).clone()                        # [nslab][Co * Ci * kk]
    ns = c["nslab"]
    if defect == "reduce_doubles_a_slab" and kk * (min(Ci, CRD_CI) // 4) <= 256:
        for k in range(0, ns // 8 * 8, 8):                      # the 8-in-flight batch of the narrow path loads slab k twice
            t[k + 1] = t[k]
    if defect == "reduce_loses_ci0":
        v = t.view(ns, Co, Ci, kk)
        for ci0 in range(CRD_CI, Ci, CRD_CI):
            cn = min(CRD_CI, Ci - ci0)
            v[:, :, ci0:ci0 + cn] = v[:, :, :cn].clone()
    return finish32(chain32(t), c["scale"], data[1], defect)


# ---- gather_frames / kind 5 ---------------------------------------------------------------------------------------------------------------

def ga(fe, counter=None, nb=1, bad=False):
    return dict(id=f"fe{fe}-" + ("nocounter" if counter is None else f"c{counter % 1000}of{nb}") + ("-badplan" if bad else ""),
                fe=fe, rows=3, table_rows=5, nb=nb, counter=counter, bad=bad)


GATHER_CASES = [ga(4), ga(1200, 5, 3), ga(4096, (1 << 63) + 1, 5), ga(16384, 5, 3), ga(1200, None, 3), ga(4, 7, 3, bad=True),
                ga(4096, None, 1, bad=True)]


def gather_gx(fe):
    vec = fe // 4
    return 8 if vec >= 4096 else (4 if vec >= 1024 else 1)


def gather_data(c):
    """(table [table_rows][fe] int32 patterns, plan [nb][rows] int64)."""
    g = gen_of(8, c["fe"], c["nb"])
    _, pat = B.SENTINEL[F]
    table = torch.randint(-2 ** 31, 2 ** 31 - 1, (c["table_rows"], c["fe"]), generator=g, dtype=torch.int64).to(torch.int32)
    table[table == pat] = 0
    plan = torch.stack([torch.randperm(c["table_rows"], generator=g)[:c["rows"]] for _ in range(c["nb"])]).to(torch.int64)
    if c["bad"]:
        b = gather_batch(c)
        plan[b, 0], plan[b, 2] = -1, c["table_rows"]
    return table, plan


def gather_batch(c):
    return 0 if c["counter"] is None else c["counter"] % c["nb"]            # the counter is unsigned


def gather_ref(c, data):
    table, plan = data
    src = plan[gather_batch(c)].clone()
    src[(src < 0) | (src >= c["table_rows"])] = 0
    return table[src]


def emu_gather(c, data, defect=None):
    table, plan = data
    _, pat = B.SENTINEL[F]
    b = 0 if defect == "gather_ignores_counter" else gather_batch(c)
    src = plan[b].clone()
    if defect == "gather_follows_bad_plan":                   # reads the guard rows around the table
        guard = torch.full((1, c["fe"]), pat, dtype=torch.int32)
        return torch.cat([guard, table, guard])[(src + 1).clamp(0, c["table_rows"] + 1)]
    src[(src < 0) | (src >= c["table_rows"])] = 0
    return table[src]


def check_gather(c, data, got, what):
    want = gather_ref(c, data)
    assert got.dtype == torch.int32 and got.shape == want.shape, (what, got.dtype, got.shape)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} words differ, first at (row {int(bad[0, 0])}, word {int(bad[0, 1])})"
    return 0.0


# ---- skinny_linear ------------------------------------------------------------------------------------------------------------------------

def sk(dt, M, Nc, K, pad=(0, 0, 0), bias=True, ksplit=1):
    es = ES[dt]
    lda, ldb, ldo = K + pad[0] * (16 // es), K + pad[1] * (16 // es), Nc + pad[2]
    return dict(id=f"{DTN[dt]}-M{M}-N{Nc}-K{K}" + (f"-parts{ksplit}" if ksplit > 1 else "") + ("" if bias else "-nobias"),
                dt=dt, M=M, Nc=Nc, K=K, lda=lda, ldb=ldb, ldo=ldo, bias=bias, ksplit=ksplit)


SKINNY_CASES = [
    sk(F32_T, 1, 1, 16, bias=False), sk(F32_T, 16, 16, 128), sk(F32_T, 17, 25, 1024, pad=(1, 2, 3)), sk(F32_T, 37, 128, 1040, pad=(2, 0, 0)),
    sk(F32_T, 37, 25, 1040, pad=(0, 1, 7), bias=False),
    sk(BF16_T, 1, 25, 32), sk(BF16_T, 16, 1, 256, pad=(1, 1, 1), bias=False), sk(BF16_T, 17, 16, 2048), sk(BF16_T, 37, 128, 2080, pad=(0, 3, 0)),
    sk(BF16_T, 17, 25, 2080, pad=(1, 0, 5)),
    sk(F32_T, 17, 25, 128, pad=(1, 0, 3), ksplit=2), sk(F32_T, 16, 16, 1040, ksplit=5), sk(F32_T, 1, 128, 1024, ksplit=2, bias=False),
    sk(BF16_T, 37, 25, 256, pad=(0, 1, 7), ksplit=2), sk(BF16_T, 17, 16, 2080, ksplit=5), sk(BF16_T, 16, 1, 2048, ksplit=2, bias=False),
]


def skinny_ks(dt):
    return 16 if dt == F32_T else 32


def skinny_branch(c):
    return f"skinny_linear_k<{DTN[c['dt']]}>" + ("[parts]" if c["ksplit"] > 1 else "")


def skinny_data(c):
    g = gen_of(9, c["M"], c["Nc"], c["K"], c["dt"])
    t = TDT[c["dt"]]
    return signed(g, c["M"], c["K"], dtype=t), signed(g, c["Nc"], c["K"], dtype=t), (signed(g, c["Nc"]) if c["bias"] else None)


SKINNY_TAIL = 16                                                 # sentinel rows behind the last part (a store past M lands there)


def emu_skinny(c, data, defect=None):
    """[ksplit * M + SKINNY_TAIL][ldo] inside sentinels: part z at rows z * M .. (z + 1) * M."""
    A, Bm, bias = data
    M, Nc, K, ksplit = c["M"], c["Nc"], c["K"], c["ksplit"]
    KS, kper = skinny_ks(c["dt"]), K // ksplit
    out = sentinel((ksplit * M + SKINNY_TAIL, c["ldo"]))
    mw = 4 if c["dt"] == F32_T else 32                            # k per MFMA
    for z in range(ksplit):
        part = torch.zeros(8, M, Nc)
        kend = kper // (64 * KS) * (64 * KS) if defect == "skinny_drops_k_tail" else kper
        for s in range(kend // KS):                               # step s belongs to wave s % 8; a wave takes its steps in order
            k0 = z * kper + s * KS
            a, b = A[:, k0:k0 + KS], Bm[:, k0:k0 + KS]
            if c["dt"] == F32_T:                                  # lane group g holds k = 4 g + q: MFMA q multiplies k = q, 4 + q, ..
                for q in range(4):
                    part[s % 8] = part[s % 8] + a[:, q::4] @ b[:, q::4].t()
            else:
                part[s % 8] = part[s % 8] + a @ b.t()
        t = chain32(part)
        if bias is not None and (z == 0 or defect == "skinny_bias_in_every_part"):
            t = t + bias[None]
        out[z * M:(z + 1) * M, :Nc] = t
        if defect == "skinny_writes_clamped_rows":
            pad = cdiv(M, 16) * 16 - M
            out[(z + 1) * M:(z + 1) * M + pad, :Nc] = t[:1]
    return out


def check_skinny(c, data, got, what):
    A, Bm, bias = data
    M, Nc, ksplit = c["M"], c["Nc"], c["ksplit"]
    kper = c["K"] // ksplit
    written = torch.zeros(got.shape, dtype=torch.bool)
    written[:ksplit * M, :Nc] = True
    check_written(got, written, what)
    worst = 0.0
    for z in range(ksplit):
        a, b = A[:, z * kper:(z + 1) * kper].to(D), Bm[:, z * kper:(z + 1) * kper].to(D)
        ref, S = a @ b.t(), a.abs() @ b.abs().t()
        if bias is not None and z == 0:
            ref, S = ref + bias.to(D)[None], S + bias.to(D).abs()[None]
        worst = max(worst, B.check(got[z * M:(z + 1) * M, :Nc], ref, S, out_dtype=F, K=kper, what=f"{what} part {z}"))
    return worst


# ---- state_vote ---------------------------------------------------------------------------------------------------------------------------

def vc(F_, L, n_states, special=None):
    return dict(id=f"F{F_}-L{L}-S{n_states}" + (f"-{special}" if special else ""), F=F_, L=L, n_states=n_states, special=special)


VOTE_CASES = ([vc(F_, L, 3) for F_, L in ((1, 1), (255, 31), (256, 32), (257, 33), (700, 100), (300, 128))]
              + [vc(12, 33, 2, "tie"), vc(40, 64, 4, "empty-state"), vc(60, 32, 3, "stray-labels"), vc(50, 40, 2, "half-and-nan")])
ONES, ZEROS = (1.0, 0.75, 0.5 + 2.0 ** -24), (0.0, 0.25, -1.0)


def vote_data(c):
    """(codes [F][L] f32, labels [F] int32)."""
    F_, L, S = c["F"], c["L"], c["n_states"]
    g = gen_of(10, F_, L, S)
    protos = torch.rand(4, L, generator=g) > 0.5                   # shared by the states: the same code occurs in several
    pick = torch.randint(0, 4, (F_,), generator=g)
    bits = protos[pick]
    labels = torch.randint(0, S, (F_,), generator=g).to(torch.int32)
    if c["special"] == "tie":                                      # state 0: codes A < B (element 0 decides), three frames each
        a, b = protos[0].clone(), protos[0].clone()
        a[0], b[0], b[1:] = False, True, ~protos[0][1:]
        bits = torch.stack([b, a, b, a, b, a] + [protos[1]] * (F_ - 6))
        labels = torch.tensor([0] * 6 + [1] * (F_ - 6), dtype=torch.int32)
    if c["special"] == "empty-state":
        labels[labels == 2] = 3
    if c["special"] == "stray-labels":
        labels[::7], labels[3::11] = -1, S
    one = torch.tensor(ONES)[torch.randint(0, 3, bits.shape, generator=g)]
    zero = torch.tensor(ZEROS)[torch.randint(0, 3, bits.shape, generator=g)]
    codes = torch.where(bits, one, zero)
    if c["special"] == "half-and-nan":                             # neither sets a bit
        z = (~bits).nonzero()
        codes[z[::2, 0], z[::2, 1]] = 0.5
        codes[z[1::2, 0], z[1::2, 1]] = float("nan")
    return codes, labels


def pack_keys(bits, lsb_first=False):
    """[F][L] bool -> [F][4] int64 words (uint32 values): element j at bit 31 - (j & 31) of word j >> 5."""
    F_, L = bits.shape
    p = np.zeros((F_, 128), dtype=np.int64)
    p[:, :L] = bits
    sh = np.arange(32) if lsb_first else 31 - np.arange(32)
    return (p.reshape(F_, 4, 32) << sh).sum(-1)


def vote_ref(c, data):
    """dict(keys [F][4], counts [F], out [S][2], winners {state: code bits}) by np.unique per state."""
    codes, labels = data[0].numpy(), data[1].numpy()
    with np.errstate(invalid="ignore"):
        bits = codes > 0.5
    keys = pack_keys(bits)
    out, winners = np.zeros((c["n_states"], 2), dtype=np.int64), {}
    for s in range(c["n_states"]):
        rows = bits[labels == s]
        if rows.shape[0]:
            uniq, cnt = np.unique(rows, axis=0, return_counts=True)
            out[s] = (cnt.max(), rows.shape[0])
            winners[s] = uniq[np.argmax(cnt)]
    same = (keys[:, None] == keys[None]).all(-1) & (labels[:, None] == labels[None])
    return dict(keys=keys, counts=same.sum(1), out=out, winners=winners)


def emu_vote(c, data, defect=None):
    """The three kernels step by step on integers."""
    codes, labels = data[0].numpy(), data[1].numpy()
    with np.errstate(invalid="ignore"):
        bits = codes >= 0.5 if defect == "vote_ge_half" else codes > 0.5
    keys = pack_keys(bits, lsb_first=defect == "vote_lsb_first")
    kt = [tuple(int(w) for w in k) for k in keys]
    F_ = len(kt)
    counts = np.array([sum(1 for j in range(F_) if kt[j] == kt[f] and (defect == "vote_counts_across_states" or labels[j] == labels[f]))
                       for f in range(F_)], dtype=np.int64)
    out, winners = np.zeros((c["n_states"], 2), dtype=np.int64), {}
    for s in range(c["n_states"]):
        best, bk, n = 0, None, 0
        for f in range(F_):
            if labels[f] != s:
                continue
            n += 1
            better = kt[f] > bk if defect == "vote_ties_to_largest" and bk is not None else (bk is None or kt[f] < bk)
            if counts[f] > best or (counts[f] == best and better):
                best, bk = int(counts[f]), kt[f]
        out[s] = (best, n)
        if bk is not None:
            w = np.array(bk, dtype=np.int64)
            winners[s] = ((w[:, None] >> (31 - np.arange(32))) & 1).reshape(-1)[:c["L"]].astype(bool)
    return dict(keys=keys, counts=counts, out=out, winners=winners)


def check_vote(c, data, got, what):
    """got: dict(keys, counts, out[, winners]) of integers."""
    ref = vote_ref(c, data)
    for k in ("keys", "counts", "out"):
        g = np.asarray(got[k], dtype=np.int64).reshape(ref[k].shape)
        if k == "keys":
            g = g & 0xFFFFFFFF
        bad = np.argwhere(g != ref[k])
        assert bad.shape[0] == 0, f"{what}: {k} differ at {bad[0].tolist()}: got {g[tuple(bad[0])]}, want {ref[k][tuple(bad[0])]}"
    if "winners" in got:
        assert set(got["winners"]) == set(ref["winners"]), what
        for s, w in ref["winners"].items():
            assert np.array_equal(np.asarray(got["winners"][s]), w), f"{what}: state {s} voted for another code than np.unique + argmax"
    return 0.0


def vote_consistency(c, out):
    """(average, per-state share) as rbvae_oracle.state_consistency reports them, from out [S][2]."""
    out = np.asarray(out, dtype=np.float64).reshape(-1, 2)
    pct = [float(a / n) if n else 0.0 for a, n in out]
    tot = out[:, 1].sum()
    return (float(np.dot(pct, out[:, 1]) / tot) if tot else 0.0), pct


# ---- the mixed job table -------------------------------------------------------------------------------------------------------------------

def table_jobs():
    """[(kind, case, dtype or None)] of the mixed table, kinds interleaved."""
    per_kind = [
        [(0, c, (F32_T, BF16_T)[i % 2]) for i, c in enumerate(PACK_CASES) if c["job"]] + [(0, c, (BF16_T, F32_T)[i % 2]) for i, c in enumerate(PACK_CASES) if c["job"]],
        [(1, c, None) for c in PERMUTE_CASES if c["job"]], [(2, c, None) for c in ROWS2_CASES], [(3, c, c["dt"]) for c in CONVPACK_CASES],
        [(4, c, None) for c in CONVRED_CASES], [(5, c, None) for c in GATHER_CASES]]
    out, k = [], 0
    while any(per_kind):
        if per_kind[k % 6]:
            out.append(per_kind[k % 6].pop(0))
        k += 1
    return out


def table_row(kind, c, dt, src=0, dst=0, dst2=0, plan=0, counter=0):
    """The row of one table entry for the given addresses (src before any offset of the case)."""
    if kind == 0:
        return job_row(0, src, dst, c["dims"], c["strides"], dtype=dt)
    if kind == 1:
        return job_row(1, src, dst, c["dims"], c["strides"], nslab=c["nslab"], slab=c["slab"], acc=c["acc"], scale=c["scale"])
    if kind == 2:
        return rows2_row(c, src, dst)
    if kind == 3:
        return job_row(3, src, dst, c["dims"], dtype=dt, dst2=dst2)
    if kind == 4:
        return job_row(4, src, dst, c["dims"], nslab=c["nslab"], slab=c["slab"], acc=c["acc"], scale=c["scale"])
    return job_row(5, src, dst, (c["rows"], c["nb"], c["fe"] // 4), (plan, counter, c["table_rows"]))


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------------

LAYOUT_BRANCHES = [
    "pack3_k<f32>", "pack3_k<bf16>", "pack3_k<f32>[grid-stride]", "pack3_k<bf16>[grid-stride]", "permute_reduce_k", "cast_pad_k<f32>",
    "cast_pad_k<bf16>", "colsum_partial_k<f32>", "colsum_partial_k<bf16>", "colsum_partial_vec_k<f32>", "colsum_partial_vec_k<bf16>",
    "colsum_final_k", "skinny_linear_k<f32>", "skinny_linear_k<bf16>", "skinny_linear_k<f32>[parts]", "skinny_linear_k<bf16>[parts]",
    "gather_frames_k[gx=1]", "gather_frames_k[gx=4]", "gather_frames_k[gx=8]", "vote_pack_k+vote_count_k+vote_pick_k",
    "run_jobs_k[0,inner]", "run_jobs_k[0,fast0]", "run_jobs_k[0,fast1]", "run_jobs_k[0,fast2]",
    "run_jobs_k[1,inner]", "run_jobs_k[1,inner,4slabs]", "run_jobs_k[1,fast0]", "run_jobs_k[1,fast1]", "run_jobs_k[1,fast2]",
    "run_jobs_k[2,wave]", "run_jobs_k[2,wide]",
    "run_jobs_k[3,vec,f32]", "run_jobs_k[3,vec,bf16]", "run_jobs_k[3,elem,f32]", "run_jobs_k[3,elem,bf16]", "run_jobs_k[3,vec,f32,split]",
    "run_jobs_k[3,vec,bf16,split]", "run_jobs_k[4,na1]", "run_jobs_k[4,na3]", "run_jobs_k[4,na4]", "run_jobs_k[4,na3,ncb]",
    "run_jobs_k[4,na1,ncb]", "run_jobs_k[5]"]


def covered_branches():
    got = {pack_branch(c, dt) for c in PACK_CASES for dt in (F32_T, BF16_T)}
    got |= {"permute_reduce_k", "colsum_final_k", "vote_pack_k+vote_count_k+vote_pick_k"}
    got |= {f"cast_pad_k<{DTN[c['dt']]}>" for c in CASTPAD_CASES} | {colsum_branch(c) for c in COLSUM_CASES}
    got |= {skinny_branch(c) for c in SKINNY_CASES} | {f"gather_frames_k[gx={gather_gx(c['fe'])}]" for c in GATHER_CASES}
    got |= {job_branch(table_row(k, c, dt)) for k, c, dt in table_jobs()}
    return got
