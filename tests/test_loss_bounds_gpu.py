"""Element-wise float64 bounds and guarded stores for the loss and optimiser kernels (tests/_loss_cases.py holds the cases,
the float64 references, the derived error model and the f32 emulations; tests/_bounds.py the buffers):

  csrc/losses.hip   binarize_kl_fwd_k, binarize_kl_fwd_parts_k, binarize_kl_bwd_k, kl_fwd_k, kl_bwd_k, pairdist_fwd_k / _bwd_k,
                    paircos_fwd_k / _bwd_k, contrast_term_fwd_k / _bwd_k / _fused_k, triplet_fwd_k / _bwd_k,
                    triplet_term_fwd_k / _bwd_k, mse_partial_k + mse_final_k, mse_bwd_k, counter_add_k
  csrc/layout.hip   combine_losses_k (with and without the hyper terms), adam_k, adam_hyper_k
  csrc/jobs.hip     run_jobs_k kinds 3-with-context (vector, element, split rows), 6 (flat and every class of the tiled
                    path) and 7, through rbvae_run_jobs and rbvae_run_jobs_sized

Every output sits inside NaN sentinels (assert_guards after every launch: no stray store, every declared element written),
every input inside NaN guard rows with NaN padding columns where the entry point takes a row stride.  The flat buffers of
the update jobs keep sentinel gaps between their tensors.  Refusals return the error and write nothing.

Worst |err| / bound per quantity, smallest .. largest over the cases, as each case prints it (BOUNDS ... worst |err|/bound),
measured on one MI355X with the library from before the shared-step pass over losses.hip (the library after it printed the
same 107 lines, character for character; 126 passed in 5.7 s):
  pairdist        fwd 7.1e-08 .. 0.046    dx1 0.018 .. 0.951     dx2 0.018 .. 0.948
  paircos         fwd 0 .. 0.043          dx1 0 .. 0.208         dx2 0 .. 0.214
  contrast_term   fwd 0.00049 .. 0.045    dh0 0.076 .. 0.532     dh1 0.426 .. 0.995      parts 0.027 .. 0.187
  triplet         fwd 0 .. 0.016          da 0 .. 0.942          dp 0 .. 0.975           dn 0 .. 0.982
  triplet_term    fwd 0 .. 0.040          dh0 0 .. 0.287         dh1 0 .. 0.301
  binarize_kl     y 0.0095 .. 0.729       kl_mean 0.0028 .. 0.080  kl_parts 0.0031 .. 0.096  bwd 0.0025 .. 0.964
  kl              fwd 0.0044 .. 0.030     bwd 0.0037 .. 0.319
  mse             fwd 0.0035 .. 0.053     bwd 0 .. 0.493
  combine_losses  recon 0.0085 .. 0.116   kl 0.0032 .. 0.088     pair 0.0056 .. 0.051    total 0.11 .. 0.373
                  hyper0 0.366 .. 0.797   hyper1 0 .. 0.903
  adam_step       w 0.499 .. 0.998        m 0.221 .. 0.963       v 0.146 .. 0.966        hyper0 0.366 .. 0.797  hyper1 0.047 .. 0.903
  update_jobs     w 0.955 .. 0.997        m 0.937 .. 0.961       v 0.920 .. 0.990
  engine          w 0.993 .. 0.998        m 0.949 .. 0.962       v 0.981 .. 0.995
The reduced values (fwd, parts, kl_mean) stay below 0.2 of their bounds, which take the worst-case growth of a sum; the
element-wise quantities reach 0.93 - 0.998, where the f32 emulation of test_loss_bounds_cpu.py put them (0.2 - 1.0).  That file also establishes, without
a device: every named defect fails, and the gradient model equals torch.autograd of the oracle."""
import struct
from importlib import import_module

import numpy as np
import pytest
import torch

import _bounds as B
import _loss_cases as C
import rbvae_oracle as O

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
ids = lambda cases: [c["id"] for c in cases]
CALLED = {}


@pytest.fixture(scope="module")
def lib():
    import sfv_amd
    return sfv_amd._lib


def call(lib, table, name, *args):
    CALLED.setdefault(table, set()).add(name)
    lib.call(name, *args)
    torch.cuda.synchronize()


def report(kind, c, res):
    res = " ".join(f"{k} {v:.3g}" for k, v in res.items()) if isinstance(res, dict) else f"{res:.3g}"
    print(f"\nBOUNDS {kind} {c} worst |err|/bound = {res}")


def rows_in(x, ld):
    """[rows][L] input with row stride ld inside NaN guard rows and NaN padding columns."""
    return B.poisoned(x, ld, F32)


def rows_out(R, ld, L, prev=None):
    g = B.guarded(R, ld, L, F32)
    return g.fill(prev.cuda()) if prev is not None else g


def flat(t, dtype=F32):
    """A contiguous input (or preloaded output) of any length inside NaN guards."""
    g = B.GuardedFlat(t.numel(), dtype)
    g.view.copy_(t.reshape(-1).to(dtype))
    return g


def flat_out(n, dtype=F32):
    return B.GuardedFlat(n, dtype)


def scalar_dev(x):
    return None if x is None else flat(torch.tensor([x], dtype=F32))


def ptr(g):
    return None if g is None else g.view


def cpu(g, shape=None):
    t = g.out.float().cpu() if g.dtype == BF else g.out.cpu()
    return t if shape is None else t.reshape(shape)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32).cpu()


def guards(what, *gs):
    for g in gs:
        if g is not None:
            B.assert_guards(g, what)


def untouched(*gs):
    for g in gs:
        ib, pat = B.SENTINEL[g.dtype]
        assert bool((g.buf.view(ib) == pat).all()), "a refused call wrote to its output"


def counter(value):
    """A device uint64 between two sentinels; returns (buffer, pointer to the middle element)."""
    buf = torch.tensor([0x5EED5EED, value, 0x5EED5EED], dtype=torch.int64, device="cuda")
    return buf, buf.data_ptr() + 8


def counter_ok(buf, want):
    v = buf.cpu().tolist()
    assert v[0] == v[2] == 0x5EED5EED, "a store next to the device counter"
    assert v[1] == (want if want < 2 ** 63 else want - 2 ** 64), (v[1], want)


# ---- pairwise distance and cosine ---------------------------------------------------------------------------------------

def _pair_bwd(lib, table, entry, c, x1, x2, nulls, acc):
    R, L = c["rows"], c["L"]
    a, b = rows_in(x1, c["s1"]), rows_in(x2, c["s2"])
    gs = scalar_dev(c["gs"])
    p1 = C.prev_of(c, "dx1", x1.shape) if acc else None
    p2 = C.prev_of(c, "dx2", x1.shape) if acc else None
    d1 = None if "dx1" in nulls else rows_out(R, c["ds1"], L, p1)
    d2 = None if "dx2" in nulls else rows_out(R, c["ds2"], L, p2)
    args = [a.view, b.view, c["s1"], c["s2"], R, L, c["label"], c["margin"], c["eps"], c["scale"], ptr(gs), ptr(d1), ptr(d2),
            c["ds1"], c["ds2"]]
    call(lib, table, entry, *(args + ([acc] if entry == "rbvae_pairdist_bwd" else [])))
    guards(f"{c['id']} {entry} nulls={nulls}", d1, d2)
    return d1 and cpu(d1), d2 and cpu(d2), p1, p2


@pytest.mark.parametrize("c", C.PAIR_CASES, ids=ids(C.PAIR_CASES))
def test_pairdist_bounded_and_guarded(lib, c):
    x1, x2 = C.pair_data(c)
    a, b, out = rows_in(x1, c["s1"]), rows_in(x2, c["s2"]), flat_out(1)
    call(lib, "PAIR_CASES", "rbvae_pairdist_fwd", a.view, b.view, c["s1"], c["s2"], c["rows"], c["L"], c["label"], c["margin"],
         c["eps"], out.view)
    guards(c["id"], out)
    res = {"fwd": C.check_pairdist_fwd(x1, x2, c["label"], c["margin"], c["eps"], cpu(out)[0], what=c["id"])}
    g1, g2, p1, p2 = _pair_bwd(lib, "PAIR_CASES", "rbvae_pairdist_bwd", c, x1, x2, c["nulls"], c["acc"])
    res.update(C.check_pairdist_bwd(x1, x2, c["label"], c["margin"], c["eps"], c["scale"], c["gs"], g1, g2, p1, p2, what=c["id"]))
    for t in (g1, g2):
        assert t is None or bool(torch.isfinite(t).all()), f"{c['id']}: NaN / inf in a gradient"
    report("pairdist", c["id"], res)


@pytest.mark.parametrize("nulls", [(), ("dx1",), ("dx2",), ("dx1", "dx2")], ids=lambda n: "null-" + "-".join(n) if n else "none")
@pytest.mark.parametrize("acc", [0, 1])
def test_pairdist_every_null_subset(lib, nulls, acc):
    c = dict(C.PAIR_CASES[2], acc=acc)
    x1, x2 = C.pair_data(c)
    g1, g2, p1, p2 = _pair_bwd(lib, "PAIR_CASES", "rbvae_pairdist_bwd", c, x1, x2, nulls, acc)
    C.check_pairdist_bwd(x1, x2, c["label"], c["margin"], c["eps"], c["scale"], c["gs"], g1, g2, p1, p2, what=f"{c['id']} {nulls}")


@pytest.mark.parametrize("c", C.COS_CASES, ids=ids(C.COS_CASES))
def test_paircos_bounded_and_guarded(lib, c):
    x1, x2 = C.cos_data(c)
    a, b, out = rows_in(x1, c["s1"]), rows_in(x2, c["s2"]), flat_out(1)
    call(lib, "COS_CASES", "rbvae_paircos_fwd", a.view, b.view, c["s1"], c["s2"], c["rows"], c["L"], c["label"], c["margin"],
         c["eps"], out.view)
    guards(c["id"], out)
    res = {"fwd": C.check_paircos_fwd(x1, x2, c["label"], c["margin"], c["eps"], cpu(out)[0], what=c["id"])}
    for nulls in {c["nulls"], ()}:
        g1, g2, _, _ = _pair_bwd(lib, "COS_CASES", "rbvae_paircos_bwd", c, x1, x2, nulls, 0)
        res.update(C.check_paircos_bwd(x1, x2, c["label"], c["margin"], c["eps"], c["scale"], c["gs"], g1, g2, what=c["id"]))
        for t in (g1, g2):
            assert t is None or bool(torch.isfinite(t).all()), f"{c['id']}: NaN / inf in a gradient"
    report("paircos", c["id"], res)


# ---- the trainer terms -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", C.TERM_CASES, ids=ids(C.TERM_CASES))
def test_contrast_term_bounded_and_guarded(lib, c):
    Bn, T, L = c["B"], c["T"], c["L"]
    h0, h1 = C.term_data(c)
    a, b, out, gs = flat(h0), flat(h1), flat_out(1), scalar_dev(c["gs"])
    call(lib, "TERM_CASES", "rbvae_contrast_term_fwd", a.view, b.view, Bn, T, L, out.view)
    guards(c["id"], out)
    res = {"fwd": C.check_contrast_fwd(h0, h1, cpu(out)[0], what=c["id"])}
    d0, d1 = flat_out(Bn * T * L), flat_out(Bn * T * L)
    call(lib, "TERM_CASES", "rbvae_contrast_term_bwd", a.view, b.view, Bn, T, L, c["scale"], ptr(gs), d0.view, d1.view)
    guards(c["id"] + " bwd", d0, d1)
    res.update(C.check_contrast_bwd(h0, h1, c["scale"], c["gs"], cpu(d0), cpu(d1), what=c["id"]))
    assert bool(torch.isfinite(cpu(d0)).all())
    n = lib.query("rbvae_contrast_term_nparts", Bn, T)
    assert n == C.cdiv(Bn * T, 4)
    parts, f0, f1 = flat_out(2 * n), flat_out(Bn * T * L), flat_out(Bn * T * L)
    call(lib, "TERM_CASES", "rbvae_contrast_term_fused", a.view, b.view, Bn, T, L, c["scale"], ptr(gs), parts.view, f0.view, f1.view)
    guards(c["id"] + " fused", parts, f0, f1)
    assert torch.equal(bits(f0.out), bits(d0.out)) and torch.equal(bits(f1.out), bits(d1.out)), "fused gradient != two-launch form"
    res["parts"] = C.check_contrast_parts(h0, h1, cpu(parts), what=c["id"])
    report("contrast_term", c["id"], res)


@pytest.mark.parametrize("c", C.TERM_CASES, ids=ids(C.TERM_CASES))
def test_triplet_term_bounded_and_guarded(lib, c):
    Bn, T, L = c["B"], c["T"], c["L"]
    h0, h1 = C.term_data(c)
    a, b, out, gs = flat(h0), flat(h1), flat_out(1), scalar_dev(c["gs"])
    call(lib, "TERM_CASES", "rbvae_triplet_term_fwd", a.view, b.view, Bn, T, L, c["margin"], out.view)
    guards(c["id"], out)
    res = {"fwd": C.check_triplet_term_fwd(h0, h1, c["margin"], cpu(out)[0], what=c["id"])}
    d0, d1 = flat_out(Bn * T * L), flat_out(Bn * T * L)
    call(lib, "TERM_CASES", "rbvae_triplet_term_bwd", a.view, b.view, Bn, T, L, c["margin"], c["scale"], ptr(gs), d0.view, d1.view)
    guards(c["id"] + " bwd", d0, d1)
    assert bool(torch.isfinite(cpu(d0)).all()) and bool(torch.isfinite(cpu(d1)).all())
    res.update(C.check_triplet_term_bwd(h0, h1, c["margin"], c["scale"], c["gs"], cpu(d0), cpu(d1), what=c["id"]))
    report("triplet_term", c["id"], res)


def _triplet_bwd(lib, c, a, p, n, nulls, acc):
    R, L = c["rows"], c["L"]
    ins = [rows_in(x, s) for x, s in zip((a, p, n), c["s"])]
    gs = scalar_dev(c["gs"])
    prev = {k: C.prev_of(c, k, a.shape) for k in "apn"} if acc else None
    outs = {k: None if k in nulls else rows_out(R, ds, L, prev[k] if acc else None) for k, ds in zip("apn", c["ds"])}
    call(lib, "TRIPLET_CASES", "rbvae_triplet_bwd", *[g.view for g in ins], *c["s"], R, L, c["margin"], c["eps"], c["swap"], c["scale"],
         ptr(gs), *[ptr(outs[k]) for k in "apn"], *c["ds"], acc)
    guards(f"{c['id']} nulls={nulls}", *outs.values())
    got = {k: (None if g is None else cpu(g)) for k, g in outs.items()}
    for t in got.values():
        assert t is None or bool(torch.isfinite(t).all())
    return got, prev


@pytest.mark.parametrize("c", C.TRIPLET_CASES, ids=ids(C.TRIPLET_CASES))
def test_triplet_bounded_and_guarded(lib, c):
    a, p, n = C.triplet_data(c)
    ins, out = [rows_in(x, s) for x, s in zip((a, p, n), c["s"])], flat_out(1)
    call(lib, "TRIPLET_CASES", "rbvae_triplet_fwd", *[g.view for g in ins], *c["s"], c["rows"], c["L"], c["margin"], c["eps"], c["swap"],
         out.view)
    guards(c["id"], out)
    res = {"fwd": C.check_triplet_fwd(a, p, n, c["margin"], c["eps"], c["swap"], cpu(out)[0], what=c["id"])}
    got, prev = _triplet_bwd(lib, c, a, p, n, c["nulls"], c["acc"])
    res.update(C.check_triplet_bwd(a, p, n, c["margin"], c["eps"], c["swap"], c["scale"], c["gs"], got, prev, what=c["id"]))
    report("triplet", c["id"], res)


NULL3 = [tuple(k for k, on in zip("apn", m) if on) for m in np.ndindex(2, 2, 2)]


@pytest.mark.parametrize("nulls", NULL3, ids=lambda n: "null-" + "".join(n) if n else "none")
def test_triplet_every_null_subset(lib, nulls):
    for acc in (0, 1):
        c = dict(C.TRIPLET_CASES[2], acc=acc)
        a, p, n = C.triplet_data(c)
        got, prev = _triplet_bwd(lib, c, a, p, n, nulls, acc)
        C.check_triplet_bwd(a, p, n, c["margin"], c["eps"], c["swap"], c["scale"], c["gs"], got, prev, what=f"{c['id']} {nulls} acc={acc}")


def test_swap_tie_splits_like_torch_minimum(lib):
    """Two bitwise equal views make dpn == dan exactly; torch.minimum (the oracle's triplet_loss) sends half of the
    negative pair's gradient each way.  Both rbvae_triplet_term_bwd and rbvae_triplet_bwd against torch.autograd."""
    c = next(c for c in C.TERM_CASES if c["special"] == "equal-views")
    Bn, T, L = c["B"], c["T"], c["L"]
    h0, h1 = C.term_data(c)
    x0, x1 = h0.double().requires_grad_(), h1.double().requires_grad_()
    g0, g1 = torch.autograd.grad(O.triplet_term(x0, x1, c["margin"]) * 2.0, (x0, x1))
    a, b, d0, d1 = flat(h0), flat(h1), flat_out(Bn * T * L), flat_out(Bn * T * L)
    call(lib, "TERM_CASES", "rbvae_triplet_term_bwd", a.view, b.view, Bn, T, L, c["margin"], 2.0, None, d0.view, d1.view)
    tol = 1e-5 * float(g0.abs().max())
    assert float((cpu(d0).double() - g0.reshape(-1)).abs().max()) < tol and float((cpu(d1).double() - g1.reshape(-1)).abs().max()) < tol
    assert float(g1.abs().max()) > 100 * tol                  # the positive's share is there to be missed
    av, pv, nv = (x.reshape(-1, L).contiguous() for x in (h0[:, :-1], h1[:, :-1], h0[:, 1:]))
    R = av.shape[0]
    xs = [x.double().requires_grad_() for x in (av, pv, nv)]
    gr = torch.autograd.grad(O.triplet_loss(*xs, c["margin"]) * 2.0, xs)
    ins, outs = [flat(x) for x in (av, pv, nv)], [flat_out(R * L) for _ in range(3)]
    call(lib, "TRIPLET_CASES", "rbvae_triplet_bwd", *[g.view for g in ins], L, L, L, R, L, c["margin"], 1e-8, 1, 2.0, None,
         *[g.view for g in outs], L, L, L, 0)
    for g, want in zip(outs, gr):
        assert float((cpu(g).double() - want.reshape(-1)).abs().max()) < 1e-5 * float(gr[0].abs().max())


# ---- binarise + KL ----------------------------------------------------------------------------------------------------------------

def _parts_check(parts, z, p, eps, clamp, what):
    n = z.numel()
    full, r = n // 256, 0.0
    if full:
        r = C.check_kl_parts(parts[:full], z.reshape(-1)[:full * 256], full, p, eps, clamp, what=what)
    if n % 256:
        r = max(r, C.check_kl_parts(parts[full:], z.reshape(-1)[full * 256:], 1, p, eps, clamp, what=what + " (last block)"))
    return r


@pytest.mark.parametrize("c", C.BIN_CASES, ids=ids(C.BIN_CASES))
def test_binarize_kl_bounded_and_guarded(lib, c):
    rows, L = c["rows"], c["L"]
    n = rows * L
    h, Un, gz, prev = C.bin_data(c)
    hd, ud = flat(h), (flat(Un) if Un is not None else None)
    sd_buf, sd = (None, None)
    if c["seed_dev"] is not None:
        sd_buf, sd = counter(0)
        call(lib, "BIN_CASES", "rbvae_counter_add", sd, c["seed_dev"])                 # counter_add_k
        counter_ok(sd_buf, c["seed_dev"])
    if Un is None:
        Un = C.device_uniform(n, c["seed"], c["seed_dev"]).view(rows, L)
    tau_dev = scalar_dev(c["tau"]) if c["tau_dev"] else None
    tau_arg = 55.0 if c["tau_dev"] else c["tau"]                                      # ignored when tau_dev is given
    y, z, kl = flat_out(n), flat_out(n), flat_out(1)
    call(lib, "BIN_CASES", "rbvae_binarize_kl_fwd", hd.view, ptr(ud), y.view, z.view, kl.view, rows, L, c["tau"], c["ratio"], c["neps"],
         c["hard"], c["p"], c["keps"], c["clamp"], c["seed"], sd)
    guards(c["id"] + " fwd", y, z, kl)
    yc, zc = cpu(y, (rows, L)), cpu(z, (rows, L))
    res = {"y": C.check_binarize(h, Un, yc, zc, c["tau"], c["ratio"], c["neps"], c["hard"], what=c["id"])}
    res["kl_mean"] = C.check_kl_mean(zc, rows, c["p"], c["keps"], c["clamp"], cpu(kl)[0], what=c["id"])
    nb = lib.query("rbvae_binarize_kl_nparts", rows, L)
    assert nb == C.cdiv(n, 256)
    y2, z2, parts = flat_out(n), flat_out(n), flat_out(nb)
    call(lib, "BIN_CASES", "rbvae_binarize_kl_fwd_parts", hd.view, ptr(ud), y2.view, z2.view, parts.view, rows, L, tau_arg, ptr(tau_dev),
         c["ratio"], c["neps"], c["hard"], c["p"], c["keps"], c["clamp"], c["seed"], sd)
    guards(c["id"] + " parts", y2, z2, parts)
    assert torch.equal(bits(y2.out), bits(y.out)) and torch.equal(bits(z2.out), bits(z.out)), "the two binarise kernels differ"
    res["kl_parts"] = _parts_check(cpu(parts), zc, c["p"], c["keps"], c["clamp"], c["id"])
    if sd_buf is not None:
        counter_ok(sd_buf, c["seed_dev"])
    gzd, gs = (flat(gz) if gz is not None else None), scalar_dev(c["gs"])
    dh = flat(prev) if prev is not None else flat_out(n)
    call(lib, "BIN_CASES", "rbvae_binarize_kl_bwd", ptr(gzd), y.view, z.view, dh.view, c["acc"], rows, L, tau_arg, ptr(tau_dev), c["klw"],
         ptr(gs), c["p"], c["keps"], c["clamp"])
    guards(c["id"] + " bwd", dh, y, z)
    res["bwd"] = C.check_binarize_bwd(gz, yc, zc, prev, rows, c["tau"], c["klw"], c["gs"], c["p"], c["keps"], c["clamp"],
                                      cpu(dh, (rows, L)), what=c["id"])
    report("binarize_kl", c["id"], res)


@pytest.mark.parametrize("c", C.KL_CASES, ids=ids(C.KL_CASES))
def test_kl_bounded_and_guarded(lib, c):
    v = C.kl_data(c)
    q, out, dq, gs = flat(v), flat_out(1), flat_out(v.numel()), scalar_dev(c["gs"])
    call(lib, "KL_CASES", "rbvae_kl_fwd", q.view, out.view, c["rows"], c["L"], c["p"], c["eps"], c["clamp"])
    call(lib, "KL_CASES", "rbvae_kl_bwd", q.view, dq.view, c["rows"], c["L"], c["p"], c["eps"], c["clamp"], c["scale"], ptr(gs))
    guards(c["id"], out, dq)
    assert bool(torch.isfinite(cpu(dq)).all())
    res = {"fwd": C.check_kl_mean(v, c["rows"], c["p"], c["eps"], c["clamp"], cpu(out)[0], what=c["id"]),
           "bwd": C.check_kl_bwd(v, c["rows"], c["p"], c["eps"], c["clamp"], c["scale"], c["gs"], cpu(dq), what=c["id"])}
    report("kl", c["id"], res)


# ---- MSE ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", C.MSE_CASES, ids=ids(C.MSE_CASES))
def test_mse_bounded_and_guarded(lib, c):
    a, b = C.mse_data(c)
    n = c["n"]
    ad, bd, out, gs = flat(a), flat(b), flat_out(1), scalar_dev(c["gs"])
    nws = lib.query("rbvae_mse_ws_floats", n)
    ws = B.GuardedFlat(nws, F32)
    call(lib, "MSE_CASES", "rbvae_mse_fwd", ad.view, bd.view, n, out.view, ws.view)
    guards(c["id"], out)
    ib, pat = B.SENTINEL[F32]
    wb = ws.buf.view(ib).cpu().reshape(-1)
    assert bool((wb[:ws.g] == pat).all()) and bool((wb[ws.g + nws:] == pat).all()), "a store outside the MSE workspace"
    assert not bool((wb[ws.g:ws.g + C.mse_blocks(n)] == pat).any()) and bool((wb[ws.g + C.mse_blocks(n):ws.g + nws] == pat).all())
    da = flat_out(n)
    call(lib, "MSE_CASES", "rbvae_mse_bwd", ad.view, bd.view, n, c["scale"], ptr(gs), da.view)
    guards(c["id"] + " bwd", da)
    res = {"fwd": C.check_mse_fwd(a, b, cpu(out)[0], what=c["id"]), "bwd": C.check_mse_bwd(a, b, c["scale"], c["gs"], cpu(da), what=c["id"])}
    report("mse", c["id"], res)


# ---- combine_losses_k, the hyper terms ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", C.COMBINE_CASES, ids=ids(C.COMBINE_CASES))
def test_combine_losses_bounded_and_guarded(lib, c):
    d = C.combine_data(c)
    sse = flat(d["sse_ws"]) if d["sse_ws"] is not None else None
    recon = flat(d["recon"]) if d["sse_ws"] is None else None
    kl, pair, out4 = flat(d["kl"]), flat(d["pair"]), flat_out(4)
    step_buf, step_ptr, hyper, lr_dev = None, None, None, None
    if c["step"] is not None:
        step_buf, step_ptr = counter(c["step"] - 1)
        hyper = flat_out(2)
        if c["lr_dev"]:
            lr_dev = torch.tensor([float("nan"), c["lr_dev"], float("nan")], dtype=torch.float64, device="cuda")
    call(lib, "COMBINE_CASES", "rbvae_combine_losses", ptr(sse), c["nparts"], c["inv_n"], ptr(recon), kl.view, c["kl_parts"], c["kl_scale"],
         pair.view, c["pair_parts"], c["w_sim"], c["w_dis"], c["beta"], c["alpha"], out4.view, step_ptr, c["lr"],
         None if lr_dev is None else lr_dev.data_ptr() + 8, c["b1"], c["b2"], ptr(hyper))
    guards(c["id"], out4, hyper)
    res = C.check_combine(d, cpu(out4), what=c["id"])
    if c["step"] is not None:
        counter_ok(step_buf, c["step"])                                               # advanced by exactly 1
        res.update(C.check_hyper(cpu(hyper), c["lr_dev"] or c["lr"], c["b1"], c["b2"], c["step"], what=c["id"]))
    report("combine_losses", c["id"], res)


# ---- rbvae_adam_step -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", C.ADAM_CASES, ids=ids(C.ADAM_CASES))
def test_adam_step_bounded_and_guarded(lib, c):
    n = c["n"]
    g = C.gen_of(n, c["steps"], 29)
    w0, m0, v0 = C.adam_data(n, g, fresh=c["steps"] > 1)
    k = C.adam_consts(c["b1"], c["b2"], c["eps"], c["gscale"])
    w, m, v = flat(w0), flat(m0), flat(v0)
    step_buf, step_ptr = counter(c["t0"])
    hyper = flat_out(2) if c["mode"] != "step" else None
    one = torch.ones(1, device="cuda")
    res = {}
    for s in range(c["steps"]):
        t = c["t0"] + s + 1
        gr = C.adam_grad(n, g, s)
        gd = flat(gr)
        before = [cpu(x).clone() for x in (w, m, v)]
        hy = (c["lr"], c["b1"], c["b2"], c["eps"])
        if c["mode"] == "step":
            call(lib, "ADAM_CASES", "rbvae_adam_step", w.view, gd.view, m.view, v.view, n, *hy, t, c["gscale"], None, None)
            step, bc2 = C.host_hyper(c["lr"], c["b1"], c["b2"], t)
        else:
            if c["mode"] == "step_dev":                                               # adam_hyper_k advances the counter itself
                call(lib, "ADAM_CASES", "rbvae_adam_step", w.view, gd.view, m.view, v.view, n, *hy, 0, c["gscale"], step_ptr, hyper.view)
            else:                                                                     # prepared by rbvae_combine_losses
                out4 = torch.empty(4, device="cuda")
                call(lib, "ADAM_CASES", "rbvae_combine_losses", None, 0, 0.0, one, one, 0, 0.0, one, 0, 0.0, 0.0, 1.0, 1.0, out4, step_ptr,
                     c["lr"], None, c["b1"], c["b2"], hyper.view)
                call(lib, "ADAM_CASES", "rbvae_adam_step", w.view, gd.view, m.view, v.view, n, *hy, 0, c["gscale"], None, hyper.view)
            counter_ok(step_buf, t)
            guards(c["id"], hyper)
            for kk, r in C.check_hyper(cpu(hyper), c["lr"], c["b1"], c["b2"], t, what=c["id"]).items():
                res[kk] = max(res.get(kk, 0.0), r)
            step, bc2 = (float(x) for x in cpu(hyper))
        guards(f"{c['id']} step {t}", w, m, v, gd)
        assert torch.equal(bits(gd.out), bits(gr)), "the gradient was written"
        after = [cpu(x) for x in (w, m, v)]
        assert all(bool(torch.isfinite(x).all()) for x in after)
        for kk, r in C.check_adam(C.adam_ref(before[0], gr, before[1], before[2], k, step, bc2), *after, what=f"{c['id']} step {t}").items():
            res[kk] = max(res.get(kk, 0.0), r)
    report("adam_step", c["id"], res)


# ---- the fused update jobs -------------------------------------------------------------------------------------------------------------

def _f2(a, b):
    return struct.unpack("<q", struct.pack("<ff", float(a), float(b)))[0]


def _prepared_hyper(lib, table):
    q = C.JOB_CONSTS
    step_buf, step_ptr = counter(q["step"] - 1)
    hyper, one, out4 = flat_out(2), torch.ones(1, device="cuda"), torch.empty(4, device="cuda")
    call(lib, table, "rbvae_combine_losses", None, 0, 0.0, one, one, 0, 0.0, one, 0, 0.0, 0.0, 1.0, 1.0, out4, step_ptr, q["lr"], None,
         q["b1"], q["b2"], hyper.view)
    return hyper


def _run_table(lib, name, sized):
    """One launch of a table in guarded flat buffers -> everything read back."""
    q = C.JOB_CONSTS
    lay, total, w0, g0, m0, v0 = C.table_data(name)
    inside = torch.zeros(total, dtype=torch.bool)
    for j, off in lay:
        inside[off:off + C.job_numel(j)] = True
    bufs = []
    for t in (w0, g0, m0, v0):
        gbuf = B.GuardedFlat(total, F32)
        gbuf.view[inside.cuda()] = t.cuda()[inside.cuda()]                            # the gaps keep the sentinel
        bufs.append(gbuf)
    w, g, m, v = bufs
    hyper = _prepared_hyper(lib, "JOB_TABLES")
    ctx = torch.tensor([w.view.data_ptr(), g.view.data_ptr(), m.view.data_ptr(), v.view.data_ptr(), hyper.view.data_ptr(),
                        _f2(1.0 - q["b1"], q["b2"]), _f2(1.0 - q["b2"], q["eps"]), _f2(q["gscale"], 0.0)], dtype=torch.int64).cuda()
    cp, rows, copies = ctx.data_ptr(), [], []
    for j, off in lay:
        src = w.view.data_ptr() + 4 * off
        n = C.job_numel(j)
        d0, d1, d2 = j["dims"]
        if j["kind"] == 7:
            rows.append([7, src, 0, n, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, cp, 0])
            copies.append([])
        elif j["kind"] == 3:
            wf, wd = flat_out(n, C.TDT[j["dtype"]]), flat_out(n, C.TDT[j["dtype"]])
            rows.append([3, src, wf.view.data_ptr(), d0, d1, d2, 0, 0, 0, 1, 0, j["dtype"], 0, 0, cp, wd.view.data_ptr()])
            copies.append([wf, wd])
        else:
            cs = [flat_out(n, C.TDT[dt]) for dt, _ in j["copies"]]
            (t1, a), (t2, b) = j["copies"][0], (j["copies"][1] if len(cs) == 2 else (0, (0, 0, 0)))
            rows.append([6, src, cs[0].view.data_ptr(), d0, d1, d2, a[0], a[1], a[2], b[0], b[1], t1 | (t2 << 8), b[2], 0, cp,
                         cs[1].view.data_ptr() if len(cs) == 2 else 0])
            copies.append(cs)
    tab = torch.tensor(rows, dtype=torch.int64).cuda()
    if sized:
        E = import_module("symbols-from-video_amd.engine")
        bmap, nb = E.job_block_map(rows, torch.device("cuda", 0), 256)
        assert 0 < nb <= 256 * len(rows) and int(bmap.view(-1, 4)[:, 0].max()) == len(rows) - 1
        call(lib, "JOB_TABLES", "rbvae_run_jobs_sized", tab, bmap, nb)
    else:
        call(lib, "JOB_TABLES", "rbvae_run_jobs", tab, len(rows), 256)
    what = f"{name} {'sized' if sized else 'plain'}"
    ib, pat = B.SENTINEL[F32]
    for nm, gbuf in zip("wgmv", bufs):
        bb = gbuf.buf.view(ib).cpu().reshape(-1)
        assert bool((bb[:gbuf.g] == pat).all()) and bool((bb[gbuf.g + total:] == pat).all()), f"{what}: a store outside the {nm} buffer"
        inner = bb[gbuf.g:gbuf.g + total]
        stray = (~inside & (inner != pat)).nonzero()
        assert stray.numel() == 0, f"{what}: {stray.numel()} elements in the gaps of {nm} were written, first at offset {int(stray[0])}"
    assert torch.equal(bits(g.view)[inside], bits(g0)[inside]), f"{what}: the gradient buffer changed"
    for cs in copies:
        guards(what + " packed copy", *cs)
    return dict(lay=lay, before=(w0, g0, m0, v0), after=tuple(x.view.cpu() for x in (w, m, v)), copies=copies,
                hyper=tuple(float(x) for x in cpu(hyper)))


@pytest.mark.parametrize("name", list(C.JOB_TABLES))
def test_update_job_tables_bounded_exact_and_guarded(lib, name):
    q = C.JOB_CONSTS
    k = C.adam_consts(q["b1"], q["b2"], q["eps"], q["gscale"])
    plain, sized = _run_table(lib, name, False), _run_table(lib, name, True)
    res = {}
    for x, y in zip(plain["after"], sized["after"]):
        assert torch.equal(bits(x), bits(y)), f"{name}: rbvae_run_jobs and rbvae_run_jobs_sized differ"
    for ca, cb in zip(plain["copies"], sized["copies"]):
        for x, y in zip(ca, cb):
            assert torch.equal(bits(x.out), bits(y.out)), f"{name}: packed copies differ between the two launch forms"
    w0, g0, m0, v0 = plain["before"]
    w1, m1, v1 = plain["after"]
    step, bc2 = plain["hyper"]
    for (j, off), cs in zip(plain["lay"], plain["copies"]):
        sl = slice(off, off + C.job_numel(j))
        r = C.check_job(j, w0[sl], g0[sl], m0[sl], v0[sl], k, step, bc2, w1[sl], m1[sl], v1[sl], [c.out.cpu() for c in cs],
                        what=f"{name}/{j['id']} {C.job_kernel(j)}")
        for kk, x in r.items():
            res[kk] = max(res.get(kk, 0.0), x)
    report("update_jobs", name, res)


ENGINE_SHAPES = [("percep", 4, "bf16", 32, (16, 16)), ("percep", 4, "f32", 25, (16, 24)), ("contrastive", 3, "bf16", 50, (32, 16)),
                 ("percep", 4, "bf16", 32, (88, 160)), ("contrastive", 3, "bf16", 25, (256, 256)), ("percep", 4, "f32", 32, (96, 128))]
PACKED = ("W1p", "W2f", "W2d", "W3f", "W3d", "Wfc", "WfcT", "Wdfc", "WdfcT", "bdfc", "V1f", "V1d", "V2f", "V2d", "V3p", "V3f", "wT_enc",
          "wT_dec")


@pytest.mark.parametrize("variant,in_ch,dtype,Ld,hw", ENGINE_SHAPES)
def test_engine_update_tables_against_float64_adam(lib, variant, in_ch, dtype, Ld, hw):
    """The six shapes of test_fused_update_jobs_equal_adam_plus_pack against the float64 Adam reference instead of adam_k;
    the packed copies equal Engine.pack of the stored masters bit for bit."""
    E = import_module("symbols-from-video_amd.engine")
    q = C.JOB_CONSTS
    k = C.adam_consts(q["b1"], q["b2"], q["eps"], q["gscale"])
    eng = E.Engine(variant, in_ch, in_ch, Ld, hw, dtype, torch.device("cuda", 0))
    n = eng.layout.total
    gen = torch.Generator().manual_seed(96)
    w0, g0 = torch.randn(n, generator=gen) * 0.1, torch.randn(n, generator=gen) * 0.01
    m0, v0 = torch.randn(n, generator=gen) * 0.01, torch.rand(n, generator=gen) * 1e-4
    w, g, m, v = (x.cuda() for x in (w0, g0, m0, v0))
    hyper = _prepared_hyper(lib, "JOB_TABLES")
    step, bc2 = (float(x) for x in cpu(hyper))
    tab, nj = eng.update_jobs(w, g, m, v, hyper.view, (q["b1"], q["b2"]), q["eps"], q["gscale"])
    eng.run_table(tab, nj)
    torch.cuda.synchronize()
    got = {kk: getattr(eng, kk).clone() for kk in PACKED}
    w1, m1, v1 = w.cpu(), m.cpu(), v.cpu()
    assert torch.equal(g.cpu(), g0)
    res, lay = {}, eng.layout
    covered = torch.zeros(n, dtype=torch.bool)
    for nm in lay.names:
        o, cnt = lay.offsets[nm], lay.view(w, nm).numel()
        sl = slice(o, o + cnt)
        covered[sl] = True
        for kk, x in C.check_adam(C.adam_ref(w0[sl], g0[sl], m0[sl], v0[sl], k, step, bc2), w1[sl], m1[sl], v1[sl], what=nm).items():
            res[kk] = max(res.get(kk, 0.0), x)
    for a, b in ((w1, w0), (m1, m0), (v1, v0)):
        assert torch.equal(a[~covered], b[~covered]), "an alignment gap of the flat buffers was written"
    eng.pack(w)
    torch.cuda.synchronize()
    for kk in PACKED:
        assert torch.equal(bits(got[kk]), bits(getattr(eng, kk))), f"{kk}: not the storage rounding of the stored master"
    report("engine update", f"{variant}-{dtype}-L{Ld}-{hw[0]}x{hw[1]}", res)


# ---- refusals: the error, and nothing written ---------------------------------------------------------------------------------------------

def test_refusals_write_nothing(lib):
    x = flat(torch.randn(4, 8))
    o1, o2, o3, s = flat_out(32), flat_out(32), flat_out(32), flat_out(1)
    nul = None

    def refused(name, *args):
        with pytest.raises(ValueError):
            lib.call(name, *args)
        torch.cuda.synchronize()
        untouched(o1, o2, o3, s)

    for T in (1, 0):                                                                   # T < 2
        refused("rbvae_contrast_term_fwd", x.view, x.view, 4, T, 8, s.view)
        refused("rbvae_contrast_term_bwd", x.view, x.view, 4, T, 8, 1.0, nul, o1.view, o2.view)
        refused("rbvae_contrast_term_fused", x.view, x.view, 4, T, 8, 1.0, nul, o3.view, o1.view, o2.view)
        refused("rbvae_triplet_term_fwd", x.view, x.view, 4, T, 8, 0.2, s.view)
        refused("rbvae_triplet_term_bwd", x.view, x.view, 4, T, 8, 0.2, 1.0, nul, o1.view, o2.view)
    for p in (0.0, 1.0, -0.1, 1.5):                                                    # p outside (0, 1)
        refused("rbvae_binarize_kl_fwd", x.view, x.view, o1.view, o2.view, s.view, 4, 8, 0.7, 0.1, 1e-8, 0, p, 1e-8, 1, 0, nul)
        refused("rbvae_binarize_kl_fwd_parts", x.view, x.view, o1.view, o2.view, s.view, 4, 8, 0.7, nul, 0.1, 1e-8, 0, p, 1e-8, 1, 0, nul)
        refused("rbvae_kl_fwd", x.view, s.view, 4, 8, p, 1e-8, 1)
        refused("rbvae_kl_bwd", x.view, o1.view, 4, 8, p, 1e-8, 1, 1.0, nul)
        refused("rbvae_binarize_kl_bwd", x.view, x.view, x.view, o1.view, 0, 4, 8, 0.7, nul, 0.3, nul, p, 1e-8, 1)
    # ... but with weight 0 the KL term and its p are not evaluated (the engine's straight-through call)
    lib.call("rbvae_binarize_kl_bwd", x.view, x.view, x.view, o1.view, 0, 4, 8, 0.7, nul, 0.0, nul, 1.0, 1e-8, 1)
    torch.cuda.synchronize()
    B.assert_guards(o1, "binarize_kl_bwd with weight 0")
    assert bool(torch.isfinite(o1.out).all())
    o1 = flat_out(32)
    for tau in (0.0, -1.0):                                                            # tau <= 0 without tau_dev
        refused("rbvae_binarize_kl_fwd", x.view, x.view, o1.view, o2.view, s.view, 4, 8, tau, 0.1, 1e-8, 0, 0.5, 1e-8, 1, 0, nul)
        refused("rbvae_binarize_kl_fwd_parts", x.view, x.view, o1.view, o2.view, s.view, 4, 8, tau, nul, 0.1, 1e-8, 0, 0.5, 1e-8, 1, 0, nul)
        refused("rbvae_binarize_kl_bwd", x.view, x.view, x.view, o1.view, 0, 4, 8, tau, nul, 0.3, nul, 0.5, 1e-8, 1)
    # nulls
    refused("rbvae_binarize_kl_fwd", nul, x.view, o1.view, o2.view, s.view, 4, 8, 0.7, 0.1, 1e-8, 0, 0.5, 1e-8, 1, 0, nul)
    refused("rbvae_binarize_kl_fwd", x.view, x.view, nul, o2.view, s.view, 4, 8, 0.7, 0.1, 1e-8, 0, 0.5, 1e-8, 1, 0, nul)
    refused("rbvae_binarize_kl_bwd", x.view, x.view, x.view, nul, 0, 4, 8, 0.7, nul, 0.3, nul, 0.5, 1e-8, 1)
    refused("rbvae_kl_fwd", nul, s.view, 4, 8, 0.5, 1e-8, 1)
    refused("rbvae_kl_bwd", x.view, nul, 4, 8, 0.5, 1e-8, 1, 1.0, nul)
    refused("rbvae_pairdist_fwd", x.view, nul, 8, 8, 4, 8, 1, 1.0, 1e-6, s.view)
    refused("rbvae_pairdist_bwd", nul, x.view, 8, 8, 4, 8, 1, 1.0, 1e-6, 1.0, nul, o1.view, o2.view, 8, 8, 0)
    refused("rbvae_paircos_fwd", x.view, x.view, 8, 8, 4, 8, 1, 1.0, 1e-8, nul)
    refused("rbvae_paircos_bwd", x.view, nul, 8, 8, 4, 8, 1, 1.0, 1e-8, 1.0, nul, o1.view, o2.view, 8, 8)
    refused("rbvae_contrast_term_bwd", x.view, x.view, 2, 2, 8, 1.0, nul, o1.view, nul)
    refused("rbvae_contrast_term_fused", x.view, x.view, 2, 2, 8, 1.0, nul, nul, o1.view, o2.view)
    refused("rbvae_triplet_fwd", x.view, x.view, nul, 8, 8, 8, 4, 8, 0.2, 1e-8, 1, s.view)
    refused("rbvae_triplet_bwd", x.view, nul, x.view, 8, 8, 8, 4, 8, 0.2, 1e-8, 1, 1.0, nul, o1.view, o2.view, o3.view, 8, 8, 8, 0)
    refused("rbvae_triplet_term_bwd", x.view, x.view, 2, 2, 8, 0.2, 1.0, nul, nul, o2.view)
    refused("rbvae_mse_fwd", x.view, x.view, 32, s.view, nul)
    refused("rbvae_mse_bwd", x.view, x.view, 32, 1.0, nul, nul)
    refused("rbvae_mse_fwd", x.view.data_ptr() + 4, x.view, 31, s.view, o1.view)       # misaligned input
    refused("rbvae_mse_fwd", x.view, x.view.data_ptr() + 8, 30, s.view, o1.view)
    # optimiser
    one = torch.ones(1, device="cuda")
    step_buf, step_ptr = counter(5)
    refused("rbvae_combine_losses", nul, 0, 0.0, one, one, 0, 0.0, one, 0, 0.0, 0.0, 1.0, 1.0, o1.view, step_ptr, 1e-3, nul, 0.9, 0.999, nul)
    refused("rbvae_combine_losses", nul, 0, 0.0, nul, one, 0, 0.0, one, 0, 0.0, 0.0, 1.0, 1.0, o1.view, nul, 1e-3, nul, 0.9, 0.999, nul)
    w = flat(torch.randn(32))
    wb = bits(w.buf)
    for args in ((0, 1.0, step_ptr, nul), (0, 1.0, nul, nul), (-3, 1.0, nul, nul)):    # step_dev without hyper_ws; neither
        refused("rbvae_adam_step", w.view, x.view, w.view, w.view, 32, 1e-3, 0.9, 0.999, 1e-8, *args)
    refused("rbvae_adam_step", w.view, nul, w.view, w.view, 32, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, nul, nul)
    assert torch.equal(bits(w.buf), wb)
    counter_ok(step_buf, 5)
    tab = torch.zeros(16, dtype=torch.int64, device="cuda")
    refused("rbvae_run_jobs", tab, 0, 256)
    refused("rbvae_run_jobs", tab, 65536, 1)
    refused("rbvae_run_jobs", tab, 1, 0)
    refused("rbvae_run_jobs", nul, 1, 256)
    bmap = torch.zeros(8, dtype=torch.int32, device="cuda")
    refused("rbvae_run_jobs_sized", tab, bmap.data_ptr() + 4, 1)                       # a misaligned block map
    refused("rbvae_run_jobs_sized", tab, bmap, 0)
    refused("rbvae_run_jobs_sized", tab, nul, 1)


# ---- coverage (runs last) ---------------------------------------------------------------------------------------------------------------

def test_tables_reach_every_kernel_and_every_entry_point_was_called():
    got = C.covered_instances()
    assert got == C.REACHABLE, (sorted(C.REACHABLE - got), sorted(got - C.REACHABLE))
    for table, names in CALLED.items():                     # of the tables that ran in this session
        want = set(C.TABLE_ENTRIES.get(table, []))
        assert want <= names, f"{table}: never called {sorted(want - names)}"
    branches = {C.job_kernel(j) for jobs in C.JOB_TABLES.values() for j in jobs}
    assert set(C.JOB_BRANCHES) == branches
