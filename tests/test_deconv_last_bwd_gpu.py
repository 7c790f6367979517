"""rbvae_deconv_last_fwd_bwd (csrc/deconv_last_bwd.hip): the last deconv's forward + sigmoid + MSE + dpre3 and the layer's
input gradient as ONE launch, against the two launches it replaces (rbvae_deconv_last_fused, then
rbvae_deconv_last_dgrad_fused) run in the same process on the same inputs.

  bit for bit      xr, dpre, every ws slot (squared-error parts and dpre column sums), dd2, col, every dd2 column-sum slot
  guards           every output starts as a NaN sentinel inside NaN guard bands (tests/_bounds.py): no stray store, every
                   declared element written, no NaN left; every input sits inside NaN guards
  independent      at 16x16, C1 = 256, Cout = 4: xr and dd2 against float64 autograd of conv_transpose2d + sigmoid + MSE on
                   the bf16-rounded operands (test_deconv_halo_gpu.py's relative bound for bf16 outputs, its constant), xr
                   and dd2 element-wise under _ends_cases' error models of the two kernels
  engine           one FusedTrainer.step with the engine switch on and off: losses, gradients and parameters equal bit for
                   bit, the captured graph one kernel node shorter

The shapes are the smallest at which the kernel can go wrong: one, two (even) and three (odd) frames; maps of two blocks per
frame (16x16), exactly one block (8x16), a block that is mostly padding (4x4) and a map no block divides (11x20); one and
four channel slices (the two instantiations) plus two and three; Cout 1 .. 4; col given and NULL; frames through the item
map [B][2][T].  d2 is a ReLU output: half of it zeros, a few negatives and -0.0, and exact zeros in every other channel on
the block borders, so that a gate taken from a neighbouring pixel shows."""
import ctypes

import pytest
import torch

import _bounds as B
import _ends_cases as E

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def lib():
    import sfv_amd
    return sfv_amd._lib


def fb(N, IH, IW, C1, Cout, col, fmap=None):
    return dict(id=f"n{N}_{IH}x{IW}_c{C1}_co{Cout}_{'col' if col else 'nocol'}{'_mapped' if fmap else ''}", N=N, IH=IH, IW=IW,
                C1=C1, Cout=Cout, col=col, fmap=fmap, gscale=0.37, gs=1.25)


CASES = [
    fb(1, 16, 16, 256, 4, True), fb(2, 16, 16, 256, 4, False, (1, 1)), fb(3, 16, 16, 64, 3, True),
    fb(1, 8, 16, 256, 3, False), fb(2, 8, 16, 64, 4, True, (1, 1)), fb(3, 8, 16, 256, 4, True),
    fb(1, 4, 4, 64, 4, False), fb(2, 4, 4, 256, 3, True, (1, 1)), fb(3, 4, 4, 256, 4, False),
    fb(1, 11, 20, 256, 4, True), fb(2, 11, 20, 64, 3, False, (1, 1)), fb(3, 11, 20, 256, 3, True),
    fb(2, 16, 16, 128, 4, True), fb(3, 16, 16, 64, 4, False), fb(2, 9, 17, 192, 2, True, (1, 1)),
    fb(1, 8, 16, 64, 1, True), fb(4, 16, 16, 256, 4, True, (1, 2)),
]
BOUND_CASE = CASES[0]


def build(c):
    """Operands on the host: d2 [N][C1][IH][IW] bf16 (ReLU-like), V [C1][Cout][3][3] bf16 and its two packed forms, bias,
    target [N][Cout][OH][OW] uniform in [0, 1)."""
    N, IH, IW, C1, Cout = c["N"], c["IH"], c["IW"], c["C1"], c["Cout"]
    g = torch.Generator().manual_seed(E.seed_of(c))
    a = torch.randn(N, C1, IH, IW, generator=g).clamp_min(0)
    flat = a.reshape(-1)
    pos = torch.arange(flat.numel())
    flat[pos % 29 == 3] = -0.5                     # not a ReLU output's value, but <= 0: gated all the same
    flat[pos % 31 == 5] = -0.0
    yy, xx = torch.arange(IH)[:, None], torch.arange(IW)[None, :]
    border = ((yy % E.TA == 0) | (yy % E.TA == E.TA - 1) | (xx % E.TB == 0) | (xx % E.TB == E.TB - 1))
    a[:, 0::2] = torch.where(border, torch.zeros(()), a[:, 0::2])
    a[:, 1::2] = torch.where(border, a[:, 1::2] + 0.25, a[:, 1::2])
    a = E.bf16r(a)
    V = E.bf16r(torch.randn(C1, Cout, 3, 3, generator=g) * 0.1)
    NYP = E.cdiv(9 * Cout, 8) * 8
    Vp = E.bf16r(torch.randn(NYP, C1, generator=g))
    Vp[:9 * Cout] = V.permute(2, 3, 1, 0).reshape(9 * Cout, C1)
    Wp = torch.zeros(C1, 64, dtype=BF)
    Wp[:, :9 * Cout] = V.permute(0, 2, 3, 1).reshape(C1, 9 * Cout)
    bias = torch.randn(Cout, generator=g)
    tgt = torch.rand(N, Cout, 2 * IH, 2 * IW, generator=g)
    return dict(a=a, V=V, Vp=Vp, Wp=Wp, NYP=NYP, bias=bias, target=tgt)


def f32_row(t):
    t = t.reshape(1, -1).float()
    return B.poisoned(t, E.cdiv(t.shape[1], 4) * 4, F32)


def flat_in(t):
    g = B.GuardedFlat(t.numel(), F32)
    g.view.copy_(t.reshape(-1).float())
    return g


def bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == BF else torch.int32).cpu()


def outputs(c, parts, nb):
    N, IH, IW, C1, Cout = c["N"], c["IH"], c["IW"], c["C1"], c["Cout"]
    P, OHW = N * IH * IW, 4 * IH * IW
    return dict(xr=B.GuardedFlat(N * Cout * OHW, F32), dpre=B.GuardedFlat(N * OHW * Cout, F32), ws=B.GuardedFlat(5 * parts, F32),
                dd2=B.guarded(P, C1, C1, BF), col=B.guarded(P, 64, 64, BF) if c["col"] else None,
                colsum=B.guarded(nb, C1, C1, F32))


def run_both(lib, c, d):
    """(two-launch outputs, one-launch outputs), each a dict of guarded buffers."""
    N, IH, IW, C1, Cout = c["N"], c["IH"], c["IW"], c["C1"], c["Cout"]
    OH, OW = 2 * IH, 2 * IW
    parts = lib.query("rbvae_deconv_last_fused_parts", 1, N, IH, IW, C1, Cout)
    nb = lib.query("rbvae_deconv_last_dgrad_blocks", 1, Cout, OH, OW, C1, N)
    assert parts == nb == N * E.cdiv(IH, E.TA) * E.cdiv(IW, E.TB)
    assert lib.query("rbvae_deconv_last_fwd_bwd_ok", 1, N, IH, IW, C1, Cout) == 1
    D2 = B.poisoned(B.rows(d["a"]), C1, BF)
    V, W = B.poisoned(d["Vp"], C1, BF), B.poisoned(d["Wp"], 64, BF)
    bias = f32_row(d["bias"])
    buf, fm = E.frame_buffer(d["target"], c["fmap"])
    tgt = flat_in(buf)
    assert (fm[0] != 0) == (c["fmap"] is not None)
    zero = torch.zeros(256, dtype=torch.uint8, device="cuda")
    two, one = outputs(c, parts, nb), outputs(c, parts, nb)
    lib.call("rbvae_deconv_last_fused", 1, D2.view, V.view, d["NYP"], bias.view, zero, N, IH, IW, C1, Cout, two["xr"].view,
             tgt.view, *fm, two["ws"].view, two["dpre"].view, c["gscale"])
    lib.call("rbvae_deconv_last_dgrad_fused", 1, two["dpre"].view, W.view, zero, two["col"] and two["col"].view, D2.view,
             two["dd2"].view, N, Cout, OH, OW, C1, C1, c["gs"], two["colsum"].view)
    lib.call("rbvae_deconv_last_fwd_bwd", 1, D2.view, V.view, d["NYP"], W.view, bias.view, zero, N, IH, IW, C1, Cout,
             one["xr"].view, tgt.view, *fm, one["ws"].view, one["dpre"].view, c["gscale"], one["col"] and one["col"].view,
             one["dd2"].view, c["gs"], one["colsum"].view)
    torch.cuda.synchronize()
    return two, one


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_one_launch_equals_two_bit_for_bit_and_guarded(lib, c):
    d = build(c)
    frac = float((d["a"].float() <= 0).float().mean())
    assert 0.4 < frac < 0.7, frac
    two, one = run_both(lib, c, d)
    for nm, g in one.items():
        if g is None:
            continue
        B.assert_guards(g, f"{c['id']} one launch {nm}")
        B.assert_guards(two[nm], f"{c['id']} two launches {nm}")
        assert not bool(torch.isnan(g.out.float()).any()), f"{c['id']}: NaN left in {nm}"
        a, b = bits(g.out), bits(two[nm].out)
        if not torch.equal(a, b):
            bad = (a != b).reshape(-1).nonzero().reshape(-1)
            raise AssertionError(f"{c['id']}: {nm} differs from the two-launch path in {bad.numel()} of {a.numel()} elements, "
                                 f"first at flat index {int(bad[0])}")
    assert float(one["dd2"].out.float().abs().max()) > 0 and float(one["dpre"].out.abs().max()) > 0


def test_against_float64_autograd(lib):
    from test_deconv_halo_gpu import DT, rel           # the relative bound of the bf16 outputs and its constant
    tol = DT["bf16"][2]
    c = BOUND_CASE
    N, IH, IW, C1, Cout = c["N"], c["IH"], c["IW"], c["C1"], c["Cout"]
    OH, OW = 2 * IH, 2 * IW
    d = build(c)
    _, one = run_both(lib, c, d)
    a = d["a"].double().requires_grad_()
    pre = torch.nn.functional.conv_transpose2d(a, d["V"].double(), d["bias"].double(), stride=2, padding=1, output_padding=1)
    xr64 = torch.sigmoid(pre)
    gscale = float(torch.tensor(c["gscale"], dtype=F32))
    (0.5 * gscale * ((xr64 - d["target"].double()) ** 2).sum()).backward()      # d/d(pre) = gscale (xr - t) xr (1 - xr)
    dd2_64 = B.rows(a.grad * float(torch.tensor(c["gs"], dtype=F32)) * (d["a"].float() > 0))
    xr = one["xr"].out.reshape(N, Cout, OH, OW).cpu()
    dd2 = one["dd2"].out.float().cpu()
    r_xr, r_dd2 = rel(xr.double(), xr64.detach()), rel(dd2.double(), dd2_64)
    print(f"\nBOUNDS deconv_last_fwd_bwd {c['id']} relative error xr {r_xr:.3g} dd2 {r_dd2:.3g} (bound {tol})")
    assert r_xr < tol and r_dd2 < tol
    # element-wise, under the error models the two kernels are held to (tests/_ends_cases.py)
    ref = dict(pre=pre.detach(), S=torch.nn.functional.conv_transpose2d(d["a"].double().abs(), d["V"].double().abs(), None, stride=2,
                                                                        padding=1, output_padding=1) + d["bias"].double().abs()[None, :, None, None],
               target=d["target"], gscale=gscale, blk=E.dl_out_blocks(c), parts=N * E.cdiv(IH, E.TA) * E.cdiv(IW, E.TB))
    parts = ref["parts"]
    got = dict(xr=xr, sse=one["ws"].out[:parts], dpre=one["dpre"].out.reshape(N, OH, OW, Cout), dsum=one["ws"].out[parts:].reshape(parts, 4))
    res = E.dl_check(c, ref, got, what=c["id"])
    x = got["dpre"].cpu().permute(0, 3, 1, 2)                                   # the STORED dpre, NCHW
    r, S = B.ref_and_scale("conv2d", E.bf16r(x), d["V"], stride=2, padding=1)
    gs = float(torch.tensor(c["gs"], dtype=F32))
    keep = B.rows(d["a"].float() > 0)
    res["dd2"] = B.check(dd2, B.rows(r) * gs * keep, B.rows(S), out_dtype=BF, K=64, scale=gs, nhw=(N, IH, IW), what=c["id"])
    assert bool((dd2[~keep] == 0).all())
    print("BOUNDS deconv_last_fwd_bwd element-wise worst |err|/bound " + " ".join(f"{k} {v:.3g}" for k, v in res.items()))


def _kernel_nodes(graph):
    hip = ctypes.CDLL("libamdhip64.so")
    n = ctypes.c_size_t(0)
    g = ctypes.c_void_p(graph.raw_cuda_graph())
    assert hip.hipGraphGetNodes(g, None, ctypes.byref(n)) == 0
    nodes = (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(g, nodes, ctypes.byref(n)) == 0
    kernels = 0
    for node in nodes:
        ty = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(ty)) == 0
        kernels += ty.value == 0                                   # hipGraphNodeTypeKernel
    return kernels


def test_trainer_step_equal_with_the_switch_on_and_off(lib, monkeypatch):
    import sfv_amd as sfv
    dbg = lib.dbg_lib()
    res = []
    g = torch.Generator().manual_seed(11)
    item = torch.rand(2, 2, 3, 4, 32, 32, generator=g).cuda()
    graph_cls = torch.cuda.CUDAGraph
    monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda *a, **k: graph_cls(keep_graph=True))
    for on in (True, False):
        torch.manual_seed(12)
        m = sfv.Seq2SeqBinaryVAE(4, 4, 32, 32, variant="percep", input_hw=(32, 32), compute_dtype="bf16").cuda().train()
        tr = sfv.FusedTrainer(m, lr=1e-3, device_noise=True, use_graph=True, seed=13)
        eng = m._engine_for(item)
        eng.deconv_last_bwd_fused = on
        losses = tr.step(item, 0.7).clone()
        torch.cuda.synchronize()
        taken = eng is tr.eng and getattr(tr.last_saved, "dd2_fused", None) is not None
        assert taken == on, "the engine switch must select the path"
        (graph,) = [gr[0] for gr in tr._graphs.values()]
        res.append((losses.cpu(), tr.gflat.clone().cpu(), m._flat.detach().clone().cpu(), _kernel_nodes(graph)))
    (l1, g1, p1, k1), (l0, g0, p0, k0) = res
    assert torch.isfinite(l1).all() and float(g1.abs().max()) > 0
    assert torch.equal(l1.view(torch.int32), l0.view(torch.int32)), (l1, l0)
    assert torch.equal(g1.view(torch.int32), g0.view(torch.int32)), int((g1 != g0).sum())
    assert torch.equal(p1.view(torch.int32), p0.view(torch.int32)), int((p1 != p0).sum())
    assert k1 == k0 - 1, (k1, k0)
    # the selector of include/rbvae_dbg_variants.h: the query answers 0 and the engine falls back to the two launches
    old = dbg.rbvae_dbg_deconv_last_variant(1)
    try:
        assert lib.query("rbvae_deconv_last_fwd_bwd_ok", 1, 12, 16, 16, 256, 4) == 0
    finally:
        dbg.rbvae_dbg_deconv_last_variant(old)
    assert lib.query("rbvae_deconv_last_fwd_bwd_ok", 1, 12, 16, 16, 256, 4) == 1
    assert lib.query("rbvae_deconv_last_fwd_bwd_ok", 0, 12, 16, 16, 256, 4) == 0          # f32
    assert lib.query("rbvae_deconv_last_fwd_bwd_ok", 1, 12, 16, 16, 320, 4) == 0          # more than four slices
    assert lib.query("rbvae_deconv_last_fwd_bwd_ok", 1, 12, 16, 16, 256, 5) == 0
