"""The keyed dropout mask (drop_mode 1: a counter hash of (seed, seed_dev[0], output element index) evaluated in the
epilogue) against its host restatement _ends_cases.keyed_keep_mask, element for element, on every template instance of
the kernels that draw it (tests/_dropout_cases.py holds the cases; test_dropout_keyed_cpu.py shows that the leading
dimension as the row pitch, a tile-local or class-local row, the bf16 walk on f32, an ignored or unmultiplied seed_dev
and a rounded threshold each change the expected mask of every case they can apply to):

  rbvae_gather_gemm        all 22 geometries of _conv_cases.GG_CASES = every (dtype, branch) of GG_REACHABLE (the column-sum
                           cases with their colsum_ws, which is part of the dispatch); dgrad rows are the class rows
  rbvae_deconv3x3s2_halo   all 12 _halo_cases.DH_CASES in the forward form = every (dtype, SC, WAVES) of DH_REACHABLE
  rbvae_conv3x3s2_halo     the five shapes of test_conv3x3s2_halo_bounded_and_guarded: both widths, the 2 x 2 image
  (rbvae_conv_first_fused  is held to the same restatement by test_ends_bounds_gpu.py, seed_dev included)

Operands are positive (rand + 0.5 in the storage type), without ReLU, gate, bias or addend, so a stored zero is exactly a
dropped element.  Every launch runs with drop_mode 0 and with drop_mode 1 at the same scale 1.25, with ldo > Nout, into
guarded outputs from poisoned inputs: (out != 0) is the restated mask on every element, the kept elements are the
drop_mode 0 run's bit for bit, the guards hold, and a repeat is bit-equal.  One case per kernel and dtype reads a device
step counter of 0, 3 and 2^40 + 1 beside a seed with its top bit set; one bf16 and one f32 gather GEMM and one case of
each halo kernel run p = 0, 2^-16, 0.1, 0.5 and 65535 / 65536 (thresh16 = 0, 1, 6553, 32768, 0xFFFF).  A trainer step
(bf16, device noise, B = 2, T = 3) at 32 x 32 frames (conv_first_fused and the gather GEMM) and at 64 x 64 with the halo
kernels' launch-size thresholds lowered (conv3x3s2_halo, deconv3x3s2_halo) is then held to the four sites' keys
noise_key * 8 + 1 .. 4 and to the device step counter, eagerly and from the captured graph; which entry point wrote each
saved activation is read from the library calls the engine made.  drop_p outside [0, 1) is refused by all four entry
points in drop_mode 1 and is not read in the other modes.

Measured on one MI355X (every test prints DROPOUT lines: the instance, the elements compared, how many differed):
  instances reached   gather_gemm_k (NT, WAVES, NS, OCC, BM): bf16 nout64_deep (2,4,3,1,64), nout64_ns1 (2,4,1,1,128),
                      nout64 (2,4,2,1,128), ns3_64sq (2,4,3,1,64), ns3_64 (1,4,3,1,128), ns3_128 (2,4,3,1,128), ns1_512
                      (2,4,1,4,128), ns1 (4,4,1,1,128), ns2 (4,8,2,1,128), ns4 (4,8,4,1,128), ns3_256 (4,8,3,1,128); f32 the
                      same without nout64_deep and ns3_64sq: 11 + 9.  deconv_halo_k<T, SC, WAVES>: (16,4), (8,4), (4,4),
                      (8,8), (4,8) in f32 and bf16.  conv_s2_k<128>, <256>.  The trainer steps: conv_first_fused + three
                      gather_gemm launches at 32 x 32; conv_first_fused, conv3x3s2_halo and two deconv3x3s2_halo launches at
                      64 x 64, eagerly and replayed.
  elements compared   119 326 016 mask elements in 55 tests (39 instance cases 36.0 M, seed_dev 1.3 M, thresholds 23.1 M, the
                      trainer steps 59.0 M)
  masks that differed none: every stored zero is a restated drop and every restated drop a stored zero, in every instance,
                      for every seed_dev and p; the replayed graph drew the eager run's masks; no kernel needed a fix
  run time            4 s for the file; the slowest test 0.7 s (the first launch of the process)
  sensitivity         a build whose gather GEMM hashed orow * ldo + col (stores unchanged) failed all 22 gather cases; the
                      trainer steps still passed it, their activations having ldo = Nout -- the pitch is the instance
                      cases' matter."""
import ctypes

import numpy as np
import pytest
import torch

import _bounds as B
import _conv_cases as C
import _dropout_cases as D
import _halo_cases as H
from _ends_cases import keyed_keep_mask

pytestmark = pytest.mark.gpu

TOP = 1 << 63


@pytest.fixture(scope="module")
def lib():
    import sfv_amd
    return sfv_amd._lib


def zero_page():
    return torch.zeros(256, dtype=torch.uint8, device="cuda")


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu()


def untouched(g):
    ib, pat = B.SENTINEL[g.dtype]
    assert bool((g.buf.view(ib) == pat).all()), "a refused call wrote to its output"


def positive(gen, rows, cols, tdt):
    return (torch.rand(rows, cols, generator=gen) + 0.5).to(tdt)


class Launch:
    """The operands of one case on the device and its launch: run(drop_mode, ...) -> the guarded output."""

    def __init__(self, lib, d):
        self.lib, self.d, c = lib, d, d["src"]
        self.tdt = tdt = C.TDT[d["dtype"]]
        g = torch.Generator().manual_seed(sum(map(ord, d["id"])))
        if d["kind"] == "gg":
            self.geom, self.desc, self.ncls, self.taps, self.Mc, rows, _, _ = C.gg_geometry(c)
            in_rows = self.geom[0] * self.geom[1] * self.geom[2]
            assert C.gg_case_instance(c)[0] == c["inst"]
            self.inst = f"gather_gemm_k<{d['dtype']}> {c['inst']} {C.gg_case_instance(c)[1]}"
            self.A = B.poisoned(positive(g, in_rows, c["Kc"], tdt), c["lda"], tdt)
            self.W = B.poisoned(positive(g, d["Nout"], self.taps * c["Kc"], tdt), self.taps * c["Kc"], tdt)
            self.cdesc = (ctypes.c_int * len(self.desc))(*self.desc)
            self.colsum = bool(c["epi"].get("colsum"))
        elif d["kind"] == "dh":
            dt, N, TH, TW, Kc, Nout = C.DTYPE_ID[c["dtype"]], c["N"], c["TH"], c["TW"], c["Kc"], c["Nout"]
            bm = H.dh_tile_rows(c["dtype"], N, TH, TW, Kc, Nout)
            assert bm and lib.query("rbvae_deconv3x3s2_halo_tile_rows", dt, N, TH, TW, Kc, Nout) == bm
            self.inst = "deconv_halo_k<%s, %d, %d>" % H.dh_instance(c)
            self.A = B.poisoned(positive(g, N * TH * TW, Kc, tdt), c["lda"], tdt)
            self.W = B.poisoned(positive(g, Nout, 9 * Kc, tdt), 9 * Kc, tdt)
        else:
            N, Kc, Nout, IH, IW = c["N"], c["Kc"], c["Nout"], c["IH"], c["IW"]
            bn = lib.query("rbvae_conv3x3s2_halo_ok", 1, N, IH, IW, Kc, Nout)
            assert bn == (256 if Nout % 256 == 0 else 128)
            self.inst = f"conv_s2_k<{bn}>"
            self.A = B.poisoned(positive(g, N * IH * IW, Kc, tdt), c["lda"], tdt)
            self.W = B.poisoned(positive(g, Nout, 9 * Kc, tdt), 9 * Kc, tdt)
        self.zero = zero_page()

    def call(self, out, drop_mode, p, seed, seed_dev, mask=None):
        d, c, lib = self.d, self.d["src"], self.lib
        Nout, ldo = d["Nout"], d["ldo"]
        if d["kind"] == "gg":
            ws = B.guarded(self.ncls * C.cdiv(self.Mc, 128), Nout, Nout, torch.float32) if self.colsum else None
            lib.call("rbvae_gather_gemm", C.DTYPE_ID[d["dtype"]], self.A.view, self.W.view, out.view, None, None, mask, None,
                     self.zero, *self.geom, c["Kc"], Nout, c["lda"], ldo, self.taps, self.ncls, ctypes.addressof(self.cdesc),
                     0, drop_mode, p, D.SCALE, seed, seed_dev, ws and ws.view)
            if ws is not None:
                torch.cuda.synchronize()
                B.assert_guards(ws, f"{d['id']} colsum_ws")
        elif d["kind"] == "dh":
            lib.call("rbvae_deconv3x3s2_halo", C.DTYPE_ID[d["dtype"]], self.A.view, self.W.view, out.view, None, None, mask,
                     self.zero, c["N"], c["TH"], c["TW"], c["Kc"], Nout, c["lda"], ldo, 0, drop_mode, p, D.SCALE, seed, seed_dev,
                     None)
        else:
            lib.call("rbvae_conv3x3s2_halo", 1, self.A.view, self.W.view, out.view, None, None, mask, c["N"], c["IH"], c["IW"],
                     c["Kc"], Nout, c["lda"], ldo, 0, drop_mode, p, D.SCALE, seed, seed_dev, None)

    def run(self, drop_mode, p=0.0, seed=0, seed_dev=None, mask=None):
        d = self.d
        out = B.guarded(d["M"], d["ldo"], d["Nout"], self.tdt)
        sd = None if seed_dev is None else torch.tensor([seed_dev], dtype=torch.int64, device="cuda")
        self.call(out, drop_mode, p, seed, sd, mask)
        torch.cuda.synchronize()
        B.assert_guards(out, f"{d['id']} {self.inst} drop_mode {drop_mode} Out")
        return out.out

    def plain(self):
        """The drop_mode 0 run: every element finite and positive, so that a zero can only be a dropped element."""
        out = self.run(0)
        v = out.float()
        assert bool(torch.isfinite(v).all()) and float(v.min()) > 0, f"{self.d['id']}: operands must give positive outputs"
        return bits(out)


TOTAL = dict(elements=0, differed=0)


@pytest.fixture(scope="module", autouse=True)
def totals():
    """After the last test of the file: what was compared (the header's figures)."""
    yield
    print(f"\nDROPOUT TOTAL: {TOTAL['elements']} elements compared, {TOTAL['differed']} differed")


def assert_mask(what, out, plain_bits, want):
    """(out != 0) is `want` on every element; kept elements are the drop_mode 0 run's bit for bit."""
    got = (out.float().cpu() != 0).numpy()
    diff = got != want
    TOTAL["elements"] += want.size
    TOTAL["differed"] += int(diff.sum())
    print(f"\nDROPOUT {what}: {want.size} elements, {int(diff.sum())} differ, {int((~want).sum())} dropped")
    if diff.any():
        r, c = np.argwhere(diff)[0]
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} mask elements differ from the restatement; first at "
                             f"(row {r}, column {c}): stored {'zero' if not got[r, c] else 'nonzero'}, restated keep {want[r, c]}; "
                             f"{len(set(np.argwhere(diff)[:, 0]))} rows, {len(set(np.argwhere(diff)[:, 1]))} columns affected")
    ob = bits(out)
    keep = torch.from_numpy(want)
    assert torch.equal(ob[keep], plain_bits[keep]), f"{what}: a kept element differs from the drop_mode 0 run"
    assert bool((ob[~keep] == 0).all()), f"{what}: a dropped element is not +0"
    return ob


@pytest.mark.parametrize("d", D.ALL_DROP, ids=[d["id"] for d in D.ALL_DROP])
def test_keyed_mask_of_every_instance(lib, d):
    L = Launch(lib, d)
    plain = L.plain()
    want = D.keep_mask(d)
    first = assert_mask(f"{d['id']} {L.inst}", L.run(1, D.P_MAIN, d["seed"]), plain, want)
    assert torch.equal(bits(L.run(1, D.P_MAIN, d["seed"])), first), f"{d['id']}: a repeat differs"


@pytest.mark.parametrize("id", D.SEED_DEV_IDS)
def test_device_step_counter_enters_the_key(lib, id):
    d = D.BY_ID[id]
    L = Launch(lib, d)
    plain = L.plain()
    seed = D.seed_of(id, top=True)
    assert seed & TOP
    null = assert_mask(f"{id} {L.inst} seed_dev NULL", L.run(1, D.P_MAIN, seed), plain, D.keep_mask(d, seed=seed))
    for v in D.SEED_DEV_VALUES:
        got = assert_mask(f"{id} {L.inst} seed_dev {v}", L.run(1, D.P_MAIN, seed, seed_dev=v), plain,
                          D.keep_mask(d, seed=seed, seed_dev=v))
        assert torch.equal(got, null) == (v == 0), f"{id}: seed_dev = {v} against the NULL mask"


@pytest.mark.parametrize("id", D.THRESH_IDS)
def test_threshold_edges(lib, id):
    d = D.BY_ID[id]
    L = Launch(lib, d)
    plain = L.plain()
    for p in D.P_EDGE:
        want = D.keep_mask(d, p=p)
        got = assert_mask(f"{id} {L.inst} p {p!r} thresh16 {D.thresh16(p):#x}", L.run(1, p, d["seed"]), plain, want)
        if p == 0.0:
            assert want.all() and torch.equal(got, plain), f"{id}: p = 0 must equal drop_mode 0"
        elif D.thresh16(p) == 1:
            assert 0 < int((~want).sum()) < want.size / 10000
        elif D.thresh16(p) == 0xFFFF:
            assert 0 < int(want.sum()) < want.size / 10000             # the few survivors, exactly the restated ones


# ---- drop_p outside [0, 1) ---------------------------------------------------------------------------------------------------

BAD_P = (1.0, -0.1, float("nan"))


@pytest.mark.parametrize("id", ["n64_bf16", "ns3_64_f32", "bf16_sc4_w4_grad", "cs_5x96x128x8x8"])
def test_drop_p_outside_the_unit_interval_is_refused_in_mode_1_only(lib, id):
    d = D.BY_ID[id]
    L = Launch(lib, d)
    plain = L.plain()
    ones = torch.ones(d["M"], d["Nout"], dtype=torch.uint8, device="cuda")
    for p in BAD_P:
        out = B.guarded(d["M"], d["ldo"], d["Nout"], L.tdt)
        with pytest.raises(ValueError, match="drop_p"):
            L.call(out, 1, p, d["seed"], None)
        torch.cuda.synchronize()
        untouched(out)
        # drop_mode 2 and 0 do not read drop_p
        assert torch.equal(bits(L.run(2, p, d["seed"], mask=ones)), plain), (id, p)
        assert torch.equal(bits(L.run(0, p, d["seed"])), plain), (id, p)


def test_conv_first_fused_refuses_drop_p_outside_the_unit_interval(lib):
    N, Cin, IH, IW, Nout = 2, 3, 15, 17, 64
    P = N * 8 * 9
    g = torch.Generator().manual_seed(5)
    x = B.GuardedFlat(N * Cin * IH * IW, torch.float32)
    x.view.copy_(torch.rand(N * Cin * IH * IW, generator=g))
    W = B.poisoned(positive(g, Nout, 64, torch.bfloat16), 64, torch.bfloat16)
    z = zero_page()

    def call(out, mode, p):
        lib.call("rbvae_conv_first_fused", 1, x.view, 0, 0, 0, 0, Cin * IH * IW, W.view, None, z, None, out.view, N, Cin, IH, IW,
                 Nout, Nout + 8, 0, mode, p, D.SCALE, 77, None)
        torch.cuda.synchronize()

    ref = B.guarded(P, Nout + 8, Nout, torch.bfloat16)
    call(ref, 0, 0.0)
    B.assert_guards(ref, "conv_first_fused Out")
    for p in BAD_P:
        out = B.guarded(P, Nout + 8, Nout, torch.bfloat16)
        with pytest.raises(ValueError, match="drop_p"):
            call(out, 1, p)
        untouched(out)
        call(out, 0, p)                                                     # not read without dropout
        B.assert_guards(out, "conv_first_fused Out")
        assert torch.equal(bits(out.out), bits(ref.out))


# ---- the step's wiring: four sites, four keys, one counter that advances -------------------------------------------------------

OUT_ARG = {"rbvae_conv_first_fused": 11, "rbvae_gather_gemm": 3, "rbvae_conv3x3s2_halo": 3, "rbvae_deconv3x3s2_halo": 3}
SITES = ("a1", "a2", "d1", "d2")


def run_trainer(lib, monkeypatch, hw, use_graph, halo, steps=3):
    """Three steps of a small percep trainer whose pre-dropout activations are all positive.  Returns per step the counter
    read before it and the four keep-masks (saved activation != 0), the trainer, and the entry point that wrote each of
    the four saved activations."""
    import sfv_amd as sfv
    B_, T_ = 2, 3
    torch.manual_seed(12)
    m = sfv.Seq2SeqBinaryVAE(4, 4, 32, 32, variant="percep", input_hw=hw, compute_dtype="bf16").cuda().train()
    lay = m._layout
    i0, i1, _ = lay.conv_idx
    with torch.no_grad():
        for name in (f"encoder_cnn.conv.{i0}", f"encoder_cnn.conv.{i1}", f"decoder_cnn.deconv.{i0}", f"decoder_cnn.deconv.{i1}"):
            lay.view(m._flat, name + ".weight").abs_()
            b = lay.view(m._flat, name + ".bias")
            b.copy_(b.abs() + 0.1)
        # the LSTM output lies in (-1, 1): the decoder fc's output stays >= 1
        lay.view(m._flat, "decoder_cnn.fc.bias").copy_(lay.view(m._flat, "decoder_cnn.fc.weight").abs().sum(1) + 1)
    item = torch.rand(B_, 2, T_, 4, *hw, generator=torch.Generator().manual_seed(11)).clamp_(1e-3, 1 - 1e-3).cuda()
    tr = sfv.FusedTrainer(m, lr=1e-4, device_noise=True, use_graph=use_graph, seed=17)
    eng = m._engine_for(item)
    if halo:
        # the halo kernels are chosen from a launch size on (engine._gemm): lowered, so that a test-sized step takes them
        eng._dh_min_wgs = eng._cs_min_wgs = 1
    calls = []
    real = lib.call

    def recording(name, *args):
        if name in OUT_ARG:
            a = args[OUT_ARG[name]]
            calls.append((a.data_ptr() if torch.is_tensor(a) else a, name))
        return real(name, *args)

    monkeypatch.setattr(lib, "call", recording)
    out = []
    for _ in range(steps):
        counter = int(tr.step_dev)
        tr.step(item, 0.7)
        torch.cuda.synchronize()
        sv = tr.last_saved
        for k in SITES:
            assert bool(torch.isfinite(getattr(sv, k).float()).all()), k
        out.append((counter, [(getattr(sv, k).float() != 0).cpu().numpy() for k in SITES]))
    monkeypatch.setattr(lib, "call", real)
    assert eng is tr.eng
    writer = dict(calls)                                                 # the last call that wrote each address
    wrote = [writer.get(getattr(tr.last_saved, k).data_ptr()) for k in SITES]
    return out, tr, wrote


@pytest.mark.parametrize("hw,halo", [((32, 32), False), ((64, 64), True)], ids=["32x32_gather", "64x64_halo"])
def test_trainer_step_keys_its_four_dropout_sites_and_advances_the_counter(lib, monkeypatch, hw, halo):
    from importlib import import_module
    key = import_module("symbols-from-video_amd.trainer").noise_key(17, 0)
    eager, tr, wrote_e = run_trainer(lib, monkeypatch, hw, False, halo)
    graph, trg, wrote_g = run_trainer(lib, monkeypatch, hw, True, halo)
    assert tr._noise_key == trg._noise_key == key and trg._graphs, "the second trainer must have replayed a captured graph"
    p = tr.v.dropout
    expect = ["rbvae_conv_first_fused"] + (["rbvae_conv3x3s2_halo"] + ["rbvae_deconv3x3s2_halo"] * 2 if halo
                                           else ["rbvae_gather_gemm"] * 3)
    assert wrote_e == expect and wrote_g == expect, (wrote_e, wrote_g)
    N = 2 * 2 * 3
    prev = None
    for step, ((counter, masks), (counter_g, masks_g)) in enumerate(zip(eager, graph)):
        assert counter == counter_g == step, "the device step counter advances by one per step, replayed or not"
        for k, (name, got) in enumerate(zip(SITES, masks), start=1):
            rows, ch = got.shape
            assert ch == 256 and rows == N * (hw[0] // (2 if name in ("a1", "d2") else 4)) ** 2
            want = keyed_keep_mask(rows, ch, key * 8 + k, p, seed_dev=counter)
            diff = int((got != want).sum())
            TOTAL["elements"] += 2 * want.size
            TOTAL["differed"] += diff + int((masks_g[k - 1] != want).sum())
            print(f"\nDROPOUT step {step} {name} by {expect[k - 1]}: {want.size} elements, {diff} differ (eager), "
                  f"{int((masks_g[k - 1] != want).sum())} differ (graph)")
            assert diff == 0, f"step {step} {name}: {diff} elements differ from the mask of key * 8 + {k}, counter {counter}"
            assert np.array_equal(masks_g[k - 1], got), f"step {step} {name}: the replayed graph drew another mask"
        small = [mk[:masks[1].shape[0]] for mk in masks]
        for i in range(4):
            for j in range(i):
                assert not np.array_equal(small[i], small[j]), f"step {step}: sites {SITES[j]} and {SITES[i]} share a mask"
        if prev is not None:
            for name, a, b in zip(SITES, prev, masks):
                assert not np.array_equal(a, b), f"step {step} {name}: the mask of the step before"
        prev = masks
