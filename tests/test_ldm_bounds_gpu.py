"""Element-wise bounds and guarded stores for the frozen LDM encoder's own kernels (tests/_ldm_cases.py holds the cases,
the restated dispatch, the float64 references and the error models; tests/_bounds.py the buffers):

  rbvae_attention            attn_flash_k<64|128|256|512, 64>, attn_flash_db_k: every element against the float64 softmax
                             attention of the bf16 operands through the dispersion bound, on six data kinds (random, peaked,
                             rising, falling, uniform, huge), N = 1..3 with every image its own K / V, the fused [rows][3C]
                             operand layout and three separate padded buffers, ldo = C and C + 8; run-to-run bit identity
                             of the prefetching kernel
  rbvae_groupnorm_swish_ws   gn_partial_k / gn_finish_k / gn_apply_vec_k (cg % 4 == 0 and cg = 2) and the fallback pair
  rbvae_groupnorm_swish      gn_stats_k / gn_apply_k by every cause: output, and the mean / rstd left in the workspace
  rbvae_groupnorm_stats      the statistics alone, tiled and fallback
  rbvae_groupnorm_apply      the apply pass from GIVEN statistics, incl. a second trip of both grid-stride loops
  rbvae_gn_affine            scale / shift against float64
  rbvae_softmax_rows, rbvae_transpose2d (bit equality), rbvae_posterior_sample

Every output, workspace and latent sits inside sentinels (assert_guards: no stray store, every declared element written);
every input inside NaN guard rows and NaN padding columns.  Refusals go through the argument checks that return before a
launch and leave the outputs untouched.  Every case prints BOUNDS <kernel> <case> worst |err|/bound = ...

Worst |err| / bound per kernel form, as measured on an MI355X (the first device run of this file; a record, not a
threshold).  Where the output is bf16 the worst element is the store's own rounding against u_out |ref|, so the ratio sits
just below 1 by construction; the peaked kind is one-hot to below the bf16 rounding, its outputs are V rows bit for bit.
  attn_flash_k<64,64>    0.945 (huge)    random 0.75  rising 0.69  falling 0.62  uniform 0.77  peaked 1.8e-4
  attn_flash_k<128,64>   0.948 (huge)    random 0.73  rising 0.71  falling 0.61  uniform 0.76  peaked 3.4e-10
  attn_flash_k<256,64>   0.951 (huge)    random 0.86  rising 0.65  falling 0.75  uniform 0.78  peaked 0
  attn_flash_k<512,64>   0.968 (huge)    random 0.87  rising 0.70  falling 0.67  uniform 0.78  peaked 0
  attn_flash_db_k        0.933 (huge)    random 0.87  rising 0.69  falling 0.61  uniform 0.77  peaked 0   (1024 tokens: 0.32)
  gn_partial_k + gn_finish_k   mean 0.080  rstd 0.0068          gn_stats_k   mean 0.156  rstd 0.0098
  gn_apply_vec_k, cg % 4 == 0  y 0.147 (f32)  0.992 (bf16)      cg = 2       y 0.053 (f32)  0.991 (bf16)
  gn_apply_k                   y 0.065 (f32)  0.994 (bf16)      gn_affine_k  scale 0.974  shift 0.564
  softmax_rows_k               0.456 (f32)  0.988 (bf16)        posterior_sample_k  0.833 (f32)  0.693 (bf16)
  transpose_k                  bit-exact on every case"""
import pytest
import torch

import _bounds as B
import _ldm_cases as L

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
ids = lambda cases: [c["id"] for c in cases]


@pytest.fixture(scope="module")
def lib():
    import sfv_amd
    return sfv_amd._lib


def report(kernel, case, res):
    if isinstance(res, dict):
        res = " ".join(f"{k} {v:.3g}" for k, v in res.items())
    else:
        res = f"{res:.3g}"
    print(f"\nBOUNDS {kernel} {case} worst |err|/bound = {res}")


def flat_in(t, dtype=F32):
    """A flat input inside NaN guards."""
    g = B.GuardedFlat(t.numel(), dtype)
    g.view.copy_(t.reshape(-1).to(dtype))
    return g


def f32_row(t):
    """A [1][n] f32 vector (gamma, beta) inside NaN guard rows, its row padded with NaN to 16 bytes."""
    t = t.reshape(1, -1).float()
    return B.poisoned(t, L.cdiv(t.shape[1], 4) * 4, F32)


def row_align(ld, dtype):
    return 16 if (ld * torch.empty((), dtype=dtype).element_size()) % 16 == 0 else 8


def untouched(*gs):
    for g in gs:
        ib, pat = B.SENTINEL[g.dtype]
        assert bool((g.buf.view(ib) == pat).all()), "a refused call wrote to its output"


def bits_of(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32).cpu()


# ---- rbvae_attention ---------------------------------------------------------------------------------------------------

def attn_operands(c, d):
    rows, C = c["N"] * c["hw"], c["C"]
    q, k, v = (d[n].reshape(rows, C) for n in "qkv")
    if c["layout"] == "fused":          # one [rows][3C] buffer, K and V as column offsets (how ldm.py calls it)
        buf = B.poisoned(torch.cat([q, k, v], 1), 3 * C, BF)
        return (buf.view, buf.view[:, C:], buf.view[:, 2 * C:]), (3 * C,) * 3, [buf]
    bufs = [B.poisoned(t, C + 8, BF) for t in (q, k, v)]
    return tuple(b.view for b in bufs), (C + 8,) * 3, bufs


@pytest.mark.parametrize("c", L.AT_CASES, ids=ids(L.AT_CASES))
def test_attention_bounded_and_guarded(lib, c):
    N, hw, C, ldo = c["N"], c["hw"], c["C"], c["ldo"]
    assert lib.query("rbvae_attention_ok", 1, hw, C) == L.attn_ok(1, hw, C) == 1
    form = L.attn_form(C, hw)
    d, _, _ = L.at_case(c["id"])
    (Q, K, V), (ldq, ldk, ldv), keep = attn_operands(c, d)
    outs = []
    for _ in range(2 if form == "attn_flash_db_k" else 1):
        o = B.guarded(N * hw, ldo, C, BF)
        lib.call("rbvae_attention", 1, Q, K, V, o.view, N, hw, C, ldq, ldk, ldv, ldo, d["scale"])
        torch.cuda.synchronize()
        B.assert_guards(o, f"{c['id']} {form} O")
        outs.append(o)
    worst = L.at_check(c, outs[0].out.float().cpu(), f"{c['id']} {form}")
    if len(outs) == 2:
        assert torch.equal(bits_of(outs[0].out), bits_of(outs[1].out)), f"{c['id']}: the prefetching kernel is not reproducible"
    report(form, c["id"], worst)


def test_attention_refusals_leave_the_output_untouched(lib):
    N, hw, C = 2, 64, 128
    x = torch.randn(N * 96, 3 * C, generator=torch.Generator().manual_seed(1)).bfloat16()
    buf = B.poisoned(x, 3 * C, BF)
    f32 = B.poisoned(x.float(), 3 * C, F32)
    Q, K, V = buf.view, buf.view[:, C:], buf.view[:, 2 * C:]
    o = B.guarded(N * 96, C + 8, C, BF)
    ld, s = 3 * C, float(C ** -0.5)
    refusals = {
        "dtype f32": (0, f32.view, f32.view[:, C:], f32.view[:, 2 * C:], o.view, N, hw, C, ld, ld, ld, C + 8, s),
        "hw = 48": (1, Q, K, V, o.view, N, 48, C, ld, ld, ld, C + 8, s),
        "C = 96": (1, Q, K, V, o.view, N, hw, 96, ld, ld, ld, C + 8, s),
        "ldq < C": (1, Q, K, V, o.view, N, hw, C, C - 8, ld, ld, C + 8, s),
        "ldk % 8": (1, Q, K, V, o.view, N, hw, C, ld, ld + 4, ld, C + 8, s),
        "ldo < C": (1, Q, K, V, o.view, N, hw, C, ld, ld, ld, C - 8, s),
        "K off by one element": (1, Q, buf.view.reshape(-1)[C + 1:], V, o.view, N, hw, C, ld, ld, ld, C + 8, s),
        "N = 0": (1, Q, K, V, o.view, 0, hw, C, ld, ld, ld, C + 8, s),
    }
    for what, args in refusals.items():
        with pytest.raises(ValueError):
            lib.call("rbvae_attention", *args)
        torch.cuda.synchronize()
        untouched(o)
    lib.call("rbvae_attention", 1, Q, K, V, o.view, N, hw, C, ld, ld, ld, C + 8, s)       # the same buffers are accepted
    torch.cuda.synchronize()
    assert not bool(torch.isnan(o.view[:N * hw, :C].float()).any())


# ---- GroupNorm ---------------------------------------------------------------------------------------------------------

def gn_operands(c, d):
    N, HW, C, dt = c["N"], c["HW"], c["C"], L.TDT[c["dtype"]]
    rows, es = N * HW, torch.empty((), dtype=L.TDT[c["dtype"]]).element_size()
    x2 = d["x"].reshape(rows, C)
    if c["misalign"] == "x":            # the data 8 bytes into every row: x % 16 == 8, ldx % V == 0
        off = 8 // es
        assert c["ldx"] >= C + off
        xb = B.guarded(rows, c["ldx"], c["ldx"], dt)
        xb.view[:, off:off + C].copy_(x2.to(dt))
        x = xb.view[:, off:]
        assert x.data_ptr() % 16 == 8
    else:
        xb = B.poisoned(x2, c["ldx"], dt, row_align=row_align(c["ldx"], dt))
        x = xb.view
    if c["misalign"] == "gamma":
        gb = B.GuardedFlat(C + 1, F32)
        gb.view[1:].copy_(d["gamma"])
        gamma = gb.view[1:]
        assert gamma.data_ptr() % 16 == 4
    else:
        gb = f32_row(d["gamma"])
        gamma = gb.view
    bb = f32_row(d["beta"])
    return x, gamma, bb.view, [xb, gb, bb]


@pytest.mark.parametrize("c", L.GN_CASES, ids=ids(L.GN_CASES))
def test_groupnorm_bounded_and_guarded(lib, c):
    N, HW, C, G, dt, dtn = c["N"], c["HW"], c["C"], c["groups"], L.TDT[c["dtype"]], L.DT[c["dtype"]]
    rows, ldx, ldy = N * HW, c["ldx"], c["ldy"]
    stats, apply, cause = L.gn_route(c)
    d, _ = L.gn_case(c["id"])
    x, gamma, beta, keep = gn_operands(c, d)
    full = lib.query("rbvae_groupnorm_ws_floats", dtn, N, HW, C, G)
    assert full == L.gn_ws_floats(c["dtype"], N, HW, C, G)
    got, y, ws = {}, None, None
    if c["entry"] != "stats":
        y = B.guarded(rows, ldy, C, dt, row_align=row_align(ldy, dt))
    if c["entry"] != "apply":
        nws = full if (c["ws"] == "full" and c["entry"] != "swish") else 2 * N * G
        ws = B.GuardedFlat(nws, F32)
        ws.view.zero_()                 # the alignment slack of the partials is never written; mean / rstd are compared
    if c["entry"] == "swish_ws":
        lib.call("rbvae_groupnorm_swish_ws", dtn, x, y.view, gamma, beta, ws.view, nws, N, HW, C, ldx, ldy, G, L.GN_EPS, c["swish"])
    elif c["entry"] == "swish":
        lib.call("rbvae_groupnorm_swish", dtn, x, y.view, gamma, beta, ws.view, N, HW, C, ldx, ldy, G, L.GN_EPS, c["swish"])
    elif c["entry"] == "stats":
        lib.call("rbvae_groupnorm_stats", dtn, x, ws.view, nws, N, HW, C, ldx, G, L.GN_EPS)
    else:
        mean, rstd = flat_in(d["mean"]), flat_in(d["rstd"])
        lib.call("rbvae_groupnorm_apply", dtn, x, y.view, mean.view, rstd.view, gamma, beta, N, HW, C, ldx, ldy, G, c["swish"])
    torch.cuda.synchronize()
    what = f"{c['id']} {stats} {apply}"
    if y is not None:
        B.assert_guards(y, f"{what} y")
        got["y"] = y.out.cpu()
    if ws is not None:
        B.assert_guards(ws, f"{what} workspace")
        got["mean"], got["rstd"] = ws.view[:N * G].cpu(), ws.view[N * G:2 * N * G].cpu()
    res = L.gn_check(c, got, what)
    report(f"{stats or '-'} {apply or '-'}", f"{c['id']} {c['dtype']}" + (f" fallback: {cause}" if cause else ""), res)


def test_groupnorm_refusals_leave_the_outputs_untouched(lib):
    N, HW, C, G = 2, 40, 128, 32
    x = B.poisoned(torch.randn(N * HW, C), C, F32)
    gamma, beta = f32_row(torch.ones(C)), f32_row(torch.zeros(C))
    y = B.guarded(N * HW, C, C, F32)
    ws = B.GuardedFlat(2 * N * G, F32)
    st = flat_in(torch.ones(N * G))
    sw = lambda dtype=0, C=C, ldx=C, ldy=C, G=G, nws=2 * N * G: lib.call(
        "rbvae_groupnorm_swish_ws", dtype, x.view, y.view, gamma.view, beta.view, ws.view, nws, N, HW, C, ldx, ldy, G, L.GN_EPS, 1)
    calls = {
        "C % groups": lambda: sw(C=100),
        "ldx < C": lambda: sw(ldx=C - 4),
        "ldy < C": lambda: sw(ldy=C - 4),
        "workspace too small": lambda: sw(nws=2 * N * G - 1),
        "dtype": lambda: sw(dtype=2),
        "groups = 0": lambda: sw(G=0),
        "swish entry, C % groups": lambda: lib.call("rbvae_groupnorm_swish", 0, x.view, y.view, gamma.view, beta.view, ws.view, N, HW,
                                                    100, C, C, G, L.GN_EPS, 1),
        "stats, workspace too small": lambda: lib.call("rbvae_groupnorm_stats", 0, x.view, ws.view, 2 * N * G - 1, N, HW, C, C, G, L.GN_EPS),
        "stats, dtype": lambda: lib.call("rbvae_groupnorm_stats", 2, x.view, ws.view, 2 * N * G, N, HW, C, C, G, L.GN_EPS),
        "stats, ldx < C": lambda: lib.call("rbvae_groupnorm_stats", 0, x.view, ws.view, 2 * N * G, N, HW, C, C - 4, G, L.GN_EPS),
        "apply, ldy < C": lambda: lib.call("rbvae_groupnorm_apply", 0, x.view, y.view, st.view, st.view, gamma.view, beta.view, N, HW,
                                           C, C, C - 4, G, 1),
        "apply, dtype": lambda: lib.call("rbvae_groupnorm_apply", 2, x.view, y.view, st.view, st.view, gamma.view, beta.view, N, HW,
                                         C, C, C, G, 1),
        "apply, C % groups": lambda: lib.call("rbvae_groupnorm_apply", 0, x.view, y.view, st.view, st.view, gamma.view, beta.view, N,
                                              HW, 100, C, C, G, 1),
    }
    for what, f in calls.items():
        with pytest.raises(ValueError):
            f()
        torch.cuda.synchronize()
        untouched(y, ws)


@pytest.mark.parametrize("c", L.AF_CASES, ids=ids(L.AF_CASES))
def test_gn_affine_bounded_and_guarded(lib, c):
    N, C, G = c["N"], c["C"], c["groups"]
    d = L.af_data(c)
    ins = [flat_in(d[k]) for k in ("mean", "rstd", "gamma", "beta")]
    scale, shift = B.GuardedFlat(N * C, F32), B.GuardedFlat(N * C, F32)
    lib.call("rbvae_gn_affine", *[g.view for g in ins], scale.view, shift.view, N, C, G)
    torch.cuda.synchronize()
    B.assert_guards(scale, f"{c['id']} scale")
    B.assert_guards(shift, f"{c['id']} shift")
    ref = L.af_reference(c, d)
    res = {k: L.check_bound(g.view.cpu().reshape(N, C), *ref[k], f"gn_affine {c['id']} {k}") for k, g in (("scale", scale), ("shift", shift))}
    report("gn_affine_k", c["id"], res)
    with pytest.raises(ValueError):
        lib.call("rbvae_gn_affine", *[g.view for g in ins], scale.view, shift.view, N, C, 7)


# ---- the small kernels -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", L.SM_CASES, ids=ids(L.SM_CASES))
def test_softmax_rows_bounded_and_guarded(lib, c):
    dt, rows, n, ld = L.TDT[c["dtype"]], c["rows"], c["n"], c["ld"]
    x = L.sm_data(c)
    ref, bnd = L.sm_reference(c, x)
    y = B.guarded(rows, ld, n, dt)
    if c["inplace"]:
        y.fill(x.cuda())
        src = y
    else:
        src = B.poisoned(x, ld, dt)
    lib.call("rbvae_softmax_rows", L.DT[c["dtype"]], src.view, y.view, rows, n, ld)
    torch.cuda.synchronize()
    B.assert_guards(y, c["id"])
    worst = L.check_bound(y.out.cpu(), ref, bnd, f"softmax_rows {c['id']}")
    report(f"softmax_rows_k<{c['dtype']}>", c["id"], worst)
    z = B.guarded(rows, ld, n, dt)
    for args in ((2, src.view, z.view, rows, n, ld), (L.DT[c["dtype"]], src.view, z.view, rows, n, n - 1),
                 (L.DT[c["dtype"]], src.view, z.view, 0, n, ld)):
        with pytest.raises(ValueError):
            lib.call("rbvae_softmax_rows", *args)
    torch.cuda.synchronize()
    untouched(z)


@pytest.mark.parametrize("c", L.TR_CASES, ids=ids(L.TR_CASES))
def test_transpose2d_is_bit_exact_and_guarded(lib, c):
    dt, R, C, ldi, ldo = L.TDT[c["dtype"]], c["R"], c["C"], c["ldi"], c["ldo"]
    bits = L.tr_bits(c)
    src = B.guarded(R, ldi, C, dt)
    src.out.view(bits.dtype).copy_(bits.cuda())
    assert torch.equal(src.out.view(bits.dtype).cpu(), bits)
    out = B.guarded(C, ldo, R, dt)
    lib.call("rbvae_transpose2d", L.DT[c["dtype"]], src.view, out.view, R, C, ldi, ldo)
    torch.cuda.synchronize()
    B.assert_guards(out, c["id"])
    assert torch.equal(out.out.view(bits.dtype).cpu(), bits.t()), f"{c['id']}: the transpose changed a bit pattern"
    report(f"transpose_k<{c['dtype']}>", c["id"], 0.0)
    z = B.guarded(C, ldo, R, dt)
    for args in ((2, src.view, z.view, R, C, ldi, ldo), (L.DT[c["dtype"]], src.view, z.view, R, C, C - 1, ldo),
                 (L.DT[c["dtype"]], src.view, z.view, R, C, ldi, R - 1)):
        with pytest.raises(ValueError):
            lib.call("rbvae_transpose2d", *args)
    torch.cuda.synchronize()
    untouched(z)


@pytest.mark.parametrize("c", L.PS_CASES, ids=ids(L.PS_CASES))
def test_posterior_sample_bounded_and_guarded(lib, c):
    dt, N, Z, HW, ld = L.TDT[c["dtype"]], c["N"], c["Z"], c["HW"], c["ld"]
    d = L.ps_data(c)
    ref, bnd = L.ps_reference(c, d)
    mom = B.poisoned(d["mom"], ld, dt)
    eps = flat_in(d["eps"]) if c["eps"] else None
    lat = B.GuardedFlat(N * Z * HW, F32)
    lib.call("rbvae_posterior_sample", L.DT[c["dtype"]], mom.view, ld, eps and eps.view, lat.view, N, Z, HW, d["scale"])
    torch.cuda.synchronize()
    B.assert_guards(lat, c["id"])
    worst = L.check_bound(lat.view.cpu(), ref, bnd, f"posterior_sample {c['id']}")
    report(f"posterior_sample_k<{c['dtype']}>", c["id"], worst)
    z = B.GuardedFlat(N * Z * HW, F32)
    for args in ((2, mom.view, ld, None, z.view, N, Z, HW, 1.0), (L.DT[c["dtype"]], mom.view, 2 * Z - 1, None, z.view, N, Z, HW, 1.0),
                 (L.DT[c["dtype"]], mom.view, ld, None, z.view, N, 0, HW, 1.0)):
        with pytest.raises(ValueError):
            lib.call("rbvae_posterior_sample", *args)
    torch.cuda.synchronize()
    untouched(z)
