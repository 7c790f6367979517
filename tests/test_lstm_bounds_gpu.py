"""Cell-by-cell float64 bounds and guarded stores for the LSTM kernels (csrc/lstm.hip) through the C ABI.
tests/_lstm_cases.py holds the restated dispatch, the case tables, the float64 references and the error model (every
stored cell against the values the kernel itself stored one step upstream); tests/_bounds.py the guarded buffers.

  rbvae_lstm_fwd / _fwd_ex     lstm_fwd_wave_k<32,*,*>, lstm_fwd_big_k<10..32>, lstm_fwd_k<32>; slabs, cast copy, inference
  rbvae_lstm_bwd / _ex / _bin  lstm_bwd_wave_k<32,*>, lstm_bwd_big_k<10..32>, lstm_bwd_k<32>; slabs, cast, column sums,
                               the fused binarise backward
  rbvae_lstm_pair_fwd / _bwd   the unit and gate-row kernels (rbvae_dbg_lstm_unit_threads), both stacks and the seam
  rbvae_lstm_wgrad / _pair     lstm_wgrad_mfma_k, every entry of the block, accumulate 0 / 1
  refusals                     the calls the dispatch says are refused return an error and write nothing

Every output sits inside NaN sentinels (nothing outside the declared elements changes, every declared element is
written); every input inside NaN guards, slab padding filled with NaN."""
import pytest
import torch

import _bounds as B
import _lstm_cases as C

pytestmark = pytest.mark.gpu

F32 = torch.float32
CAST = {"f32": (0, torch.float32), "bf16": (1, torch.bfloat16)}


@pytest.fixture(scope="module")
def lib():
    import sfv_amd
    return sfv_amd._lib


class Bufs:
    """Guarded buffers of one call: inp() poisoned inputs, out() sentinel-filled outputs, checked by guards()."""

    def __init__(self):
        self.outs, self.keep = [], []

    def inp(self, t):
        if t is None:
            return None
        g = B.GuardedFlat(t.numel(), t.dtype)
        g.view.copy_(t.reshape(-1).cuda())
        self.keep.append(g)
        return g.view

    def out(self, n, name, dtype=F32, prefill=None):
        g = B.GuardedFlat(n, dtype)
        if prefill is not None:
            g.view[:prefill.numel()].copy_(prefill.reshape(-1).cuda())
        self.outs.append((name, g))
        return g

    def guards(self, what):
        torch.cuda.synchronize()
        for name, g in self.outs:
            B.assert_guards(g, f"{what}: {name}")

    def untouched(self, what):
        torch.cuda.synchronize()
        for name, g in self.outs:
            ib, pat = B.SENTINEL[g.dtype]
            assert bool((g.buf.view(ib) == pat).all()), f"{what}: the refused call wrote into {name}"


def slabs(parts, pad):
    """[nparts][n] -> a flat [nparts][n + pad] buffer with NaN padding."""
    buf = torch.full((parts.shape[0], parts.shape[1] + pad), float("nan"))
    buf[:, :parts.shape[1]] = parts
    return buf


def cast_args(bufs, c, rows):
    if c["cast"] is None:
        return None, 0, 0, None
    dt_id, dt = CAST[c["cast"][0]]
    g = bufs.out(rows * c["cast"][1], "cast_out", dt)
    return g.view, dt_id, c["cast"][1], g


def report(kind, c, inst, worst):
    print(f"\nBOUNDS lstm {kind} {C.case_id(c)} {inst}: " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))


def finite(*ts):
    for t in ts:
        assert torch.isfinite(t.float()).all()


class unit_threads:
    def __init__(self, lib, unit):
        self.l, self.unit = lib.dbg_lib(), unit

    def __enter__(self):
        self.old = self.l.rbvae_dbg_lstm_unit_threads(self.unit)

    def __exit__(self, *a):
        self.l.rbvae_dbg_lstm_unit_threads(self.old)


# ---- forward -------------------------------------------------------------------------------------------------------

def fwd_call(lib, c, w, wT, parts, x, train):
    S, T, L, layers = c["S"], c["T"], c["L"], c["layers"]
    n = S * T * L
    b = Bufs()
    use_parts = c["nparts"] > 1 or c["pad"] > 0
    hs = b.out((layers + 1) * n, "hs_all", prefill=None if use_parts else x)
    hp, acts, cs = (b.out(layers * n, "hprev"), b.out(layers * 4 * n, "acts"), b.out(layers * n, "cs")) if train else (None,) * 3
    cast, cast_id, cast_ld, cast_g = cast_args(b, c, S * T)
    pv = lambda g: g.view if g is not None else None
    if use_parts or cast is not None:
        lib.call("rbvae_lstm_fwd_ex", b.inp(w), b.inp(wT), hs.view, pv(hp), pv(acts), pv(cs), S, T, L, layers,
                 b.inp(slabs(parts, c["pad"])) if use_parts else None, c["nparts"], n + c["pad"], cast, cast_id, cast_ld)
    else:
        lib.call("rbvae_lstm_fwd", b.inp(w), b.inp(wT), hs.view, pv(hp), pv(acts), pv(cs), S, T, L, layers)
    return b, hs, hp, acts, cs, cast_g


@pytest.mark.parametrize("c", C.FWD_CASES, ids=[C.case_id(c) for c in C.FWD_CASES])
def test_lstm_forward_cells_bounded_and_guarded(lib, c):
    S, T, L, layers = c["S"], c["T"], c["L"], c["layers"]
    inst = C.fwd_instance(c)
    assert isinstance(inst, str), inst
    assert bool(lib.query("rbvae_lstm_fwd_wave_ok", T, L, layers)) == inst.startswith("lstm_fwd_wave_k")
    gen = C.gen_for(c)
    w = C.make_weights(L, layers, c["regime"], gen)
    wT = C.make_wT(w, L, layers) if c["wT"] else None
    parts = C.make_input(c, gen)
    x = C.slab_sum_fwd(parts).reshape(S, T, L)
    b, hs, hp, acts, cs, cast_g = fwd_call(lib, c, w, wT, parts, x, True)
    what = f"{C.case_id(c)} {inst}"
    b.guards(what)
    shp = (layers, S, T, L)
    hs_c, hp_c, cs_c = hs.view.cpu().view(layers + 1, S, T, L), hp.view.cpu().view(shp), cs.view.cpu().view(shp)
    acts_c = acts.view.cpu().view(layers, S, T, 4 * L)
    finite(hs_c, hp_c, cs_c, acts_c)
    C._exact(hs_c[0], x, f"{what}: hs[0] == the input (slab sum in slab order)", ("sequence", "time", "unit"))
    worst = C.check_forward(w, hs_c, hp_c, acts_c, cs_c, L, layers, lib=C.is_lib_kernel(inst), what=what)
    if cast_g is not None:
        C.check_cast(cast_g.view.cpu().view(S * T, -1), hs_c[layers], L, f"{what}: cast_out")
    # inference mode: the saved tensors absent, the outputs bit for bit the same
    b2, hs2, _, _, _, cast2 = fwd_call(lib, c, w, wT, parts, x, False)
    b2.guards(what + " (inference)")
    C._exact(hs2.view.cpu().view(layers + 1, S, T, L), hs_c, f"{what}: inference == training", ("slot", "sequence", "time", "unit"))
    if cast_g is not None:
        assert torch.equal(cast2.view.cpu().view(torch.int16 if cast2.dtype == torch.bfloat16 else torch.int32),
                           cast_g.view.cpu().view(torch.int16 if cast2.dtype == torch.bfloat16 else torch.int32))
    report("fwd", c, inst, worst)


@pytest.mark.parametrize("c", C.FWD_REFUSALS, ids=[C.case_id(c) for c in C.FWD_REFUSALS])
def test_lstm_forward_refusals_write_nothing(lib, c):
    S, T, L, layers = c["S"], c["T"], c["L"], c["layers"]
    assert C.fwd_instance(c)[0] == "refused"
    gen = C.gen_for(c)
    w = C.make_weights(L, layers, "small", gen)
    parts = C.make_input(c, gen)
    n = S * T * L
    b = Bufs()
    hs, hp, acts, cs = b.out((layers + 1) * n, "hs_all"), b.out(layers * n, "hprev"), b.out(layers * 4 * n, "acts"), b.out(layers * n, "cs")
    cast, cast_id, cast_ld, _ = cast_args(b, c, S * T)
    with pytest.raises(ValueError):
        if c["nparts"] > 1 or cast is not None:
            lib.call("rbvae_lstm_fwd_ex", b.inp(w), None, hs.view, hp.view, acts.view, cs.view, S, T, L, layers,
                     b.inp(slabs(parts, 0)), c["nparts"], n, cast, cast_id, cast_ld)
        else:
            lib.call("rbvae_lstm_fwd", b.inp(w), None, hs.view, hp.view, acts.view, cs.view, S, T, L, layers)
    b.untouched(C.case_id(c))


# ---- backward ------------------------------------------------------------------------------------------------------

def bin_operands(c, gen, N, L):
    y = torch.rand(N, L, generator=gen).clamp(1e-3, 1 - 1e-3)
    z = (y > 0.5).float() if c["hard"] else y.clone()
    g_hs = torch.randn(N, L, generator=gen) if c["ghs"] else None
    return y, z, g_hs


def bwd_call(lib, c, w, wT, acts, cs, parts, bin_ops, b=None):
    S, T, L, layers = c["S"], c["T"], c["L"], c["layers"]
    n = S * T * L
    b = b or Bufs()
    dG, dx = b.out(layers * 4 * n, "dG"), b.out(n, "dx")
    cast, cast_id, cast_ld, cast_g = cast_args(b, c, S * T)
    sums = b.out(S * L, "dx_colsum") if c["colsum"] else None
    sv = sums.view if sums is not None else None
    if c["entry"] == "plain":
        lib.call("rbvae_lstm_bwd", b.inp(w), b.inp(wT), b.inp(acts), b.inp(cs), b.inp(parts[0]), dG.view, dx.view, S, T, L, layers)
    elif c["entry"] == "ex":
        lib.call("rbvae_lstm_bwd_ex", b.inp(w), b.inp(acts), b.inp(cs), b.inp(slabs(parts, c["pad"])), c["nparts"],
                 n + c["pad"], dG.view, dx.view, cast, cast_id, cast_ld, sv, S, T, L, layers)
    else:
        y, z, g_hs = bin_ops
        tau_dev = b.inp(torch.tensor([0.7])) if c["tau_dev"] else None
        lib.call("rbvae_lstm_bwd_bin", b.inp(w), b.inp(acts), b.inp(cs), b.inp(parts[0]), b.inp(y), b.inp(z), b.inp(g_hs),
                 9.0 if c["tau_dev"] else 0.7, tau_dev, c["klw"], 0.1, 1e-8, c["clamp"], dG.view, dx.view, cast, cast_id,
                 cast_ld, sv, S, T, L, layers)
    return b, dG, dx, cast_g, sums


@pytest.mark.parametrize("c", C.BWD_CASES, ids=[C.case_id(c) for c in C.BWD_CASES])
def test_lstm_backward_cells_bounded_and_guarded(lib, c):
    S, T, L, layers = c["S"], c["T"], c["L"], c["layers"]
    inst = C.bwd_instance(c)
    assert isinstance(inst, str), inst
    assert bool(lib.query("rbvae_lstm_bwd_wave_ok", T, L, layers)) == inst.startswith("lstm_bwd_wave_k")
    gen = C.gen_for(c, 1)
    w = C.make_weights(L, layers, c["regime"], gen)
    wT = C.make_wT(w, L, layers) if (c["wT"] and c["entry"] == "plain") else None
    acts, cs, _, _ = C.saved_state(c, w, gen)
    parts = torch.randn(c["nparts"], S * T * L, generator=gen)
    bin_ops = bin_operands(c, gen, S * T, L) if c["entry"] == "bin" else None
    b, dG, dx, cast_g, sums = bwd_call(lib, c, w, wT, acts, cs, parts, bin_ops)
    what = f"{C.case_id(c)} {inst}"
    b.guards(what)
    dG_c, dx_c = dG.view.cpu().view(layers, S, T, 4 * L), dx.view.cpu().view(S, T, L)
    finite(dG_c, dx_c)
    if c["entry"] == "bin":
        y, z, g_hs = bin_ops
        gref, E = C.gtop_bin(parts[0].double().view(S * T, L), 0.0, y, z, g_hs, 0.7, c["klw"], S * T, 0.1, 1e-8, c["clamp"])
        gref, E = gref.view(S, T, L), E.view(S, T, L)
    else:
        gref, E = C.slab_sum_bwd(parts).double().view(S, T, L), 0.0
    worst = C.check_backward(w, acts, cs, gref, E, dG_c, dx_c, L, layers, lib=C.is_lib_kernel(inst), what=what)
    if cast_g is not None:
        C.check_cast(cast_g.view.cpu().view(S * T, -1), dx_c, L, f"{what}: cast_out")
    if sums is not None:
        worst["colsum"] = C.check_colsum(sums.view.cpu().view(S, L), dx_c, f"{what}: dx_colsum")
    report("bwd", c, inst, worst)


@pytest.mark.parametrize("c", C.BWD_REFUSALS, ids=[C.case_id(c) for c in C.BWD_REFUSALS])
def test_lstm_backward_refusals_write_nothing(lib, c):
    S, T, L, layers = c["S"], c["T"], c["L"], c["layers"]
    assert C.bwd_instance(c)[0] == "refused"
    gen = C.gen_for(c, 1)
    w = C.make_weights(L, layers, "small", gen)
    n = S * T * L
    acts, cs = torch.rand(layers, S, T, 4 * L, generator=gen), torch.randn(layers, S, T, L, generator=gen)
    parts = torch.randn(c["nparts"], n, generator=gen)
    bin_ops = bin_operands(c, gen, S * T, L) if c["entry"] == "bin" else None
    b = Bufs()
    with pytest.raises(ValueError):
        bwd_call(lib, c, w, None, acts, cs, parts, bin_ops, b)
    b.untouched(C.case_id(c))


# ---- both stacks as one launch ---------------------------------------------------------------------------------------

def pair_fwd_call(lib, c, we, wd, wTe, wTd, parts, x, Un, train, b=None):
    S, T, L, layers = c["S"], c["T"], c["L"], c["layers"]
    n = S * T * L
    b = b or Bufs()
    use_parts = c["nparts"] > 1 or c["pad"] > 0
    o = {}
    for st in ("e", "d"):
        o["hs_" + st] = b.out((layers + 1) * n, "hs_" + st, prefill=x if (st == "e" and not use_parts) else None)
        for nm, k in (("hp_", 1), ("acts_", 4), ("cs_", 1)):
            o[nm + st] = b.out(layers * k * n, nm + st) if train else None
    o["y"] = b.out(n, "y_soft")
    o["kl"] = b.out(S, "kl_parts") if c["kl"] else None
    cast, cast_id, cast_ld, o["cast"] = cast_args(b, c, S * T)
    pv = lambda g: g.view if g is not None else None
    tau_dev = b.inp(torch.tensor([0.6])) if c["tau_dev"] else None
    with unit_threads(lib, c["unit"]):
        lib.call("rbvae_lstm_pair_fwd", b.inp(we), b.inp(wTe), b.inp(wd), b.inp(wTd), pv(o["hs_e"]), pv(o["hp_e"]),
                 pv(o["acts_e"]), pv(o["cs_e"]), pv(o["hs_d"]), pv(o["hp_d"]), pv(o["acts_d"]), pv(o["cs_d"]),
                 b.inp(slabs(parts, c["pad"])) if use_parts else None, c["nparts"], n + c["pad"], b.inp(Un), pv(o["y"]),
                 pv(o["kl"]), 9.0 if c["tau_dev"] else 0.6, tau_dev, 0.3, 1e-8, c["hard"], 0.1, 1e-8, c["clamp"], 1234, None,
                 cast, cast_id, cast_ld, S, T, L, layers)
        torch.cuda.synchronize()
    return b, o


@pytest.mark.parametrize("c", C.PAIR_FWD_CASES, ids=[C.case_id(c) for c in C.PAIR_FWD_CASES])
def test_lstm_pair_forward_cells_bounded_and_guarded(lib, c):
    S, T, L, layers = c["S"], c["T"], c["L"], c["layers"]
    inst = C.pair_fwd_dispatch(T, L, layers, c["unit"])
    assert isinstance(inst, str) and lib.query("rbvae_lstm_pair_fwd_ok", T, L, layers)
    gen = C.gen_for(c, 2)
    we, wd = C.make_weights(L, layers, c["regime"], gen), C.make_weights(L, layers, c["regime"], gen)
    wTe, wTd = (C.make_wT(we, L, layers), C.make_wT(wd, L, layers)) if c["wT"] else (None, None)
    parts = C.make_input(c, gen)
    x = C.slab_sum_fwd(parts).reshape(S, T, L)
    Un = torch.rand(S * T, L, generator=gen)
    b, o = pair_fwd_call(lib, c, we, wd, wTe, wTd, parts, x, Un, True)
    what = f"{C.case_id(c)} {inst}"
    b.guards(what)
    cpu = {k: (g.view.cpu() if g is not None else None) for k, g in o.items()}
    worst = {}
    for st, w in (("e", we), ("d", wd)):
        hs, hp, cs = cpu["hs_" + st].view(layers + 1, S, T, L), cpu["hp_" + st].view(layers, S, T, L), cpu["cs_" + st].view(layers, S, T, L)
        acts = cpu["acts_" + st].view(layers, S, T, 4 * L)
        finite(hs, hp, cs, acts)
        for k, v in C.check_forward(w, hs, hp, acts, cs, L, layers, what=f"{what} stack {st}").items():
            worst[f"{k}_{st}"] = v
    hs_e, hs_d = cpu["hs_e"].view(layers + 1, S, T, L), cpu["hs_d"].view(layers + 1, S, T, L)
    C._exact(hs_e[0], x, f"{what}: hs_enc[0] == the input", ("sequence", "time", "unit"))
    y = cpu["y"].view(S * T, L)
    worst["y"] = C.check_binarize(hs_e[layers], Un, y, hs_d[0].reshape(S * T, L), 0.6, 0.3, 1e-8, c["hard"], what)
    if c["kl"]:
        worst["kl"] = C.check_kl_parts(cpu["kl"], hs_d[0], S, 0.1, 1e-8, c["clamp"], what)
    if cpu["cast"] is not None:
        C.check_cast(cpu["cast"].view(S * T, -1), hs_d[layers], L, f"{what}: cast_out")
    b2, o2 = pair_fwd_call(lib, c, we, wd, wTe, wTd, parts, x, Un, False)
    b2.guards(what + " (inference)")
    for k in ("hs_e", "hs_d", "y"):
        C._exact(o2[k].view.cpu(), cpu[k], f"{what}: inference == training ({k})", ("element",))
    report("pair_fwd", c, inst, worst)


def pair_bwd_call(lib, c, we, wd, ae, ce, ad, cd, parts, gzx, y, z, g_hs, b=None):
    S, T, L, layers = c["S"], c["T"], c["L"], c["layers"]
    n = S * T * L
    b = b or Bufs()
    o = dict(dGe=b.out(layers * 4 * n, "dG_enc"), dGd=b.out(layers * 4 * n, "dG_dec"), dx=b.out(n, "dx"),
             dz=b.out(n, "dz") if c["dz"] else None)
    cast, cast_id, cast_ld, o["cast"] = cast_args(b, c, S * T)
    o["sums"] = b.out(S * L, "dx_colsum") if c["colsum"] else None
    pv = lambda g: g.view if g is not None else None
    tau_dev = b.inp(torch.tensor([0.7])) if c["tau_dev"] else None
    with unit_threads(lib, c["unit"]):
        lib.call("rbvae_lstm_pair_bwd", b.inp(we), b.inp(wd), b.inp(ae), b.inp(ce), b.inp(ad), b.inp(cd),
                 b.inp(slabs(parts, c["pad"])), c["nparts"], n + c["pad"], b.inp(gzx), b.inp(y), b.inp(z), b.inp(g_hs),
                 9.0 if c["tau_dev"] else 0.7, tau_dev, c["klw"], 0.1, 1e-8, c["clamp"], pv(o["dGe"]), pv(o["dGd"]), pv(o["dx"]),
                 pv(o["dz"]), cast, cast_id, cast_ld, pv(o["sums"]), S, T, L, layers)
        torch.cuda.synchronize()
    return b, o


def pair_bwd_data(c):
    S, T, L, layers = c["S"], c["T"], c["L"], c["layers"]
    gen = C.gen_for(c, 3)
    we, wd = C.make_weights(L, layers, c["regime"], gen), C.make_weights(L, layers, c["regime"], gen)
    ae, ce, _, _ = C.saved_state(c, we, gen)
    ad, cd, _, _ = C.saved_state(c, wd, gen)
    parts = torch.randn(c["nparts"], S * T * L, generator=gen)
    gzx = torch.randn(S * T, L, generator=gen) if c["extra"] else None
    y, z, g_hs = bin_operands(c, gen, S * T, L)
    return we, wd, ae, ce, ad, cd, parts, gzx, y, z, g_hs


@pytest.mark.parametrize("c", C.PAIR_BWD_CASES, ids=[C.case_id(c) for c in C.PAIR_BWD_CASES])
def test_lstm_pair_backward_cells_bounded_and_guarded(lib, c):
    S, T, L, layers = c["S"], c["T"], c["L"], c["layers"]
    inst = C.pair_bwd_dispatch(T, L, layers, c["unit"])
    assert isinstance(inst, str) and lib.query("rbvae_lstm_pair_bwd_ok", T, L, layers)
    we, wd, ae, ce, ad, cd, parts, gzx, y, z, g_hs = pair_bwd_data(c)
    b, o = pair_bwd_call(lib, c, we, wd, ae, ce, ad, cd, parts, gzx, y, z, g_hs)
    what = f"{C.case_id(c)} {inst}"
    b.guards(what)
    dGe, dGd = o["dGe"].view.cpu().view(layers, S, T, 4 * L), o["dGd"].view.cpu().view(layers, S, T, 4 * L)
    dx = o["dx"].view.cpu().view(S, T, L)
    dz = o["dz"].view.cpu().view(S, T, L) if o["dz"] is not None else None
    finite(dGe, dGd, dx)
    worst = {}
    # decoder stack: its top gradient is the slab sum; dz == W_ih_dec[0]^T dG_dec[0]
    for k, v in C.check_backward(wd, ad, cd, C.slab_sum_bwd(parts).double().view(S, T, L), 0.0, dGd, dz, L, layers,
                                 what=f"{what} decoder").items():
        worst[k + "_d"] = v
    # the seam: the codes' gradient from the kernel's own dG_dec[0] (+ gz_extra), through the binarise backward
    gz, E_gz = C.input_grad_ref(wd, dGd, L, layers)
    if gzx is not None:
        gz = gz + gzx.double().view(S, T, L)
        E_gz = E_gz + C.U * gz.abs()
    gref, E = C.gtop_bin(gz.view(S * T, L), E_gz.view(S * T, L), y, z, g_hs, 0.7, c["klw"], S * T, 0.1, 1e-8, c["clamp"])
    for k, v in C.check_backward(we, ae, ce, gref.view(S, T, L), E.view(S, T, L), dGe, dx, L, layers,
                                 what=f"{what} encoder").items():
        worst[k + "_e"] = v
    if o["cast"] is not None:
        C.check_cast(o["cast"].view.cpu().view(S * T, -1), dx, L, f"{what}: cast_out")
    if o["sums"] is not None:
        worst["colsum"] = C.check_colsum(o["sums"].view.cpu().view(S, L), dx, f"{what}: dx_colsum")
    report("pair_bwd", c, inst, worst)


@pytest.mark.parametrize("which,c", C.PAIR_REFUSALS, ids=[w + "-" + C.case_id(c) for w, c in C.PAIR_REFUSALS])
def test_lstm_pair_refusals_write_nothing(lib, which, c):
    S, T, L, layers = c["S"], c["T"], c["L"], c["layers"]
    gen = C.gen_for(c, 4)
    b = Bufs()
    w = C.make_weights(L, layers, "small", gen)
    with pytest.raises(ValueError):
        if which == "fwd":
            assert not lib.query("rbvae_lstm_pair_fwd_ok", T, L, layers)
            parts = C.make_input(c, gen)
            pair_fwd_call(lib, c, w, w, None, None, parts, parts[0].reshape(S, T, L), torch.rand(S * T, L, generator=gen), True, b)
        else:
            assert not lib.query("rbvae_lstm_pair_bwd_ok", T, L, layers)
            a, cc = torch.rand(layers, S, T, 4 * L, generator=gen), torch.randn(layers, S, T, L, generator=gen)
            y, z, g_hs = bin_operands(c, gen, S * T, L)
            pair_bwd_call(lib, c, w, w, a, cc, a, cc, torch.randn(1, S * T * L, generator=gen), None, y, z, g_hs, b)
    torch.cuda.synchronize()
    for name, g in b.outs:
        if not (which == "fwd" and name == "hs_e"):                # slot 0 of hs_enc is the caller's input
            ib, pat = B.SENTINEL[g.dtype]
            assert bool((g.buf.view(ib) == pat).all()), f"the refused call wrote into {name}"


# ---- weight gradient -----------------------------------------------------------------------------------------------

def wgrad_data(c, salt):
    S, T, L, layers = c["S"], c["T"], c["L"], c["layers"]
    gen = C.gen_for(c, 5 + salt)
    w = C.make_weights(L, layers, c["regime"], gen)
    hs, hp, acts, cs = C.forward_pass(w, torch.randn(S, T, L, generator=gen), L, layers)
    dG, _ = C.backward_pass(w, acts, cs, torch.randn(S, T, L, generator=gen), L, layers)
    prev = torch.randn(layers * C.layer_floats(L), generator=gen) if c["acc"] else None
    return dG, hs, hp, prev


@pytest.mark.parametrize("c", C.WGRAD_CASES, ids=[C.case_id(c) + f"-pair{int(c['pair'])}-acc{c['acc']}" for c in C.WGRAD_CASES])
def test_lstm_wgrad_every_entry_bounded_and_guarded(lib, c):
    S, T, L, layers = c["S"], c["T"], c["L"], c["layers"]
    nb = layers * C.layer_floats(L)
    stacks = [wgrad_data(c, k) for k in range(2 if c["pair"] else 1)]
    b = Bufs()
    outs = [b.out(nb, f"gblk_{k}", prefill=d[3]) for k, d in enumerate(stacks)]
    ins = [[b.inp(t) for t in d[:3]] for d in stacks]
    if c["pair"]:
        lib.call("rbvae_lstm_wgrad_pair", *ins[0], outs[0].view, *ins[1], outs[1].view, S, T, L, layers, c["acc"])
    else:
        lib.call("rbvae_lstm_wgrad", *ins[0], outs[0].view, S, T, L, layers, c["acc"])
    what = f"{C.case_id(c)} {C.wgrad_dispatch(c['pair'], c['acc'])}"
    b.guards(what)
    worst = {}
    for k, (d, g) in enumerate(zip(stacks, outs)):
        gb = g.view.cpu()
        finite(gb)
        worst[f"stack{k}"] = C.check_wgrad(d[0], d[1], d[2], gb, L, layers, prev=d[3], what=f"{what} stack {k}")
    report("wgrad", c, C.wgrad_dispatch(c["pair"], c["acc"]), worst)
