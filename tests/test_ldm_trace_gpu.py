"""Launch-by-launch float64 bounds for the LDM encoder and decoder on the device (tests/_ldm_trace_ref.py holds the cases, the
restated wiring, the references and the storage model; tests/test_ldm_trace_cpu.py checks those without a GPU).

One eager pass per case with _LDMBlocks._trace on; then, per recorded launch (its inputs and its output as the device left
them, teacher-forced: an error does not travel),
  (a) element-wise   |got - ref| <= the bound of the op: _bounds.check for the convolutions / GEMMs (K = taps Kc, pre, the
                     staged-operand term), the GroupNorm / softmax / attention bounds of _ldm_cases.py, the tile-statistics
                     bounds of _halo_cases.py; bit equality for im2col, transpose, nearest2x and latent_rows; padding columns
                     exactly zero.  f32 cases: the same calls with the f32 roundoffs.
  (b) bf16 only      relative L2 of the stored output against the reference <= 2 x the storage model's own (float64 arithmetic
                     rounded where the device stores or stages, computed here from the same recorded inputs).  The device adds
                     f32 accumulation and evaluation error (c_acc ~ 4e-7 S), orders below the bf16 roundings of the floor.
  (c) chain          the recorded (prefix, op) list is expected_stages; every input lives in an earlier record's output (or is
                     the frame / latent); the last record is what the pass returned.
  (d) guards         the latent, the image and the u8 frame are written inside NaN / 0xA5 guard bands, and moments / encode /
                     decode / decode_u8 are bit-identical with and without the trace.
Every record prints BOUNDS ldm-trace <case> <prefix> <op> worst |err|/bound = .. (rel L2 / floor = ..).

Worst per case as measured on an MI355X (a record, not a threshold): see MEASURED below."""
import pytest
import torch

import _bounds as B
import _ldm_trace_ref as T

pytestmark = pytest.mark.gpu

# worst |err| / bound over the records of a case, and worst relative L2 / floor (bf16), first device run of this file
MEASURED = """
  case                  worst |err|/bound   where                              rel L2 / floor (min .. max over the records)
  bf16_halo_2x64x64     0.996  conv_in (the bf16 store's own rounding)         0.998 .. 1.00   (0.998: attention)
  bf16_halo_3x32x128    0.996  conv_in, conv1                                  0.999 .. 1.00
  bf16_halo_1x128x128   0.996  conv_in, gn_apply                               1.00 .. 1.00
  f32_halo_2x32x64      0.630  conv1 (conv3_halo 0.39, pv 0.60, scores 0.54)   -
  f32_gather_1x64x64    0.981  conv3 (pv 0.92, conv1 0.64)                     -
  bf16_gather_1x64x64   0.996  conv_in_gemm                                    1.00 .. 1.00
  bf16_halo_2x8x8       0.996  conv1, gn_apply, up_halo 0.995                  0.997 .. 1.00   (0.997: attention)
  bf16_halo_1x4x12      0.996  gn_apply (scores 0.98, softmax 0.97, pv 0.99)   1.00 .. 1.00
  f32_gather_1x8x8      0.925  up_gather (pv 0.83, conv1 0.66)                 -
  bf16_unfolded_1x8x8   0.996  conv3 (up_unfolded 0.99)                        1.00 .. 1.00
  bf16_unfolded_1x4x4   0.994  conv1 (16 tokens padded to 64; up_unfolded 0.99)  1.00 .. 1.00
  The statistics records (f32, no storage rounding) sit far inside their bounds in every case: gn_stats <= 0.033, gn_affine <=
  0.0041, gn_finish <= 0.0033, gn_finish_ms <= 0.0029; bf16 attention 0.47 .. 0.69; im2col, transpose, nearest2x and
  latent_rows are bit-equal.  No record is above 1.00 of the floor: nothing to explain under gate (b).
"""

ids = lambda cases: [c["id"] for c in cases]


@pytest.fixture(scope="module")
def sfv():
    import sfv_amd
    return sfv_amd


def traced(m, f):
    m._trace = []
    try:
        out = f()
        torch.cuda.synchronize()
        return m._trace, out
    finally:
        m._trace = None


def check_trace(c, m, P, records, sources, last):
    """gates (a), (b), (c) over the records of one pass; every failing record is reported, not the first alone"""
    N, H, W = c["N"], c["H"], c["W"]
    stages = T.expected_stages(m, N, H, W)
    T.assert_reach(c, stages)
    assert [(r[0], r[1]) for r in records] == stages
    T.check_chain(records, sources, last)
    tdt = T.TDT[c["dtype"]]
    cpu = lambda t: None if t is None else t.detach().cpu()
    failures, worst, ratio = [], 0.0, 0.0
    for prefix, op, ins, out, g in records:
        rec = (prefix, op, tuple(cpu(t) for t in ins), tuple(cpu(t) for t in out) if isinstance(out, tuple) else cpu(out), g)
        try:
            o = T.check_record(rec, P, tdt)
        except AssertionError as e:
            failures.append(f"{prefix} {op}: {e}")
            print(f"\nBOUNDS ldm-trace {c['id']} {prefix} {op} FAILED {e}")
            continue
        worst = max(worst, o["worst"])
        line = f"\nBOUNDS ldm-trace {c['id']} {prefix} {op} worst |err|/bound = {o['worst']:.3g}"
        if o["floor"] is not None:
            ratio = max(ratio, o["l2"] / o["floor"])
            line += f" rel L2 / floor = {o['l2']:.3g} / {o['floor']:.3g} = {o['l2'] / o['floor']:.3g}"
        print(line)
    print(f"\nBOUNDS ldm-trace {c['id']} MAXIMA worst |err|/bound = {worst:.3g} rel L2 / floor = {ratio:.3g} over {len(records)} records")
    assert not failures, f"{len(failures)} of {len(records)} records outside a gate:\n" + "\n".join(failures)


@pytest.mark.parametrize("c", T.ENC_CASES, ids=ids(T.ENC_CASES))
def test_encoder_launch_by_launch(sfv, c):
    m, P = T.make_model(sfv, c)
    m = m.cuda()
    x = T.make_input(c).cuda()
    N, H, W = c["N"], c["H"], c["W"]
    eps = torch.randn(N, 4, H // 8, W // 8, generator=torch.Generator().manual_seed(3)).cuda()
    # (d) the latent inside NaN guards; with and without the trace bit for bit
    plain_m = m.moments(x).clone()
    lat = B.GuardedFlat(N * 4 * (H // 8) * (W // 8), torch.float32)
    plain = m.encode(x, eps=eps, out=lat.view).clone()
    torch.cuda.synchronize()
    B.assert_guards(lat, f"{c['id']} latent")
    records, mom = traced(m, lambda: m.moments(x))
    assert torch.equal(mom, plain_m)
    lat2 = B.GuardedFlat(lat.rows, torch.float32)
    n_rec = len(records)
    recs2, got = traced(m, lambda: m.encode(x, eps=eps, out=lat2.view))
    B.assert_guards(lat2, f"{c['id']} latent, traced")
    assert torch.equal(got, plain) and len(recs2) == n_rec
    assert m._trace is None and list(m.state_dict().keys()) == list(P.keys())
    check_trace(c, m, P, records, [x], mom)


@pytest.mark.parametrize("c", T.DEC_CASES, ids=ids(T.DEC_CASES))
def test_decoder_launch_by_launch(sfv, c):
    m, P = T.make_model(sfv, c)
    m = m.cuda()
    z = T.make_input(c).cuda()
    N, H, W = c["N"], c["H"], c["W"]
    n_img = N * 3 * 64 * H * W
    guard = 4096

    def u8_run():
        buf = torch.full((guard + n_img + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        m._check_input(z)
        m._run(z, 4, None, buf[guard:guard + n_img].view(N, 8 * H, 8 * W, 3))
        torch.cuda.synchronize()
        b = buf.cpu()
        assert bool((b[:guard] == 0xA5).all()) and bool((b[guard + n_img:] == 0xA5).all()), f"{c['id']}: a u8 store outside the frame"
        return b[guard:guard + n_img].view(N, 8 * H, 8 * W, 3)

    img = B.GuardedFlat(n_img, torch.float32)
    plain = m.decode(z, out=img.view).clone()
    torch.cuda.synchronize()
    B.assert_guards(img, f"{c['id']} image")
    assert [f for f, _, _ in m.upsample_dispatch] == list(c["forms"]), m.upsample_dispatch
    plain_u8 = u8_run()
    assert torch.equal(plain_u8, m.decode_u8(z).cpu())
    img2 = B.GuardedFlat(n_img, torch.float32)
    recs2, got = traced(m, lambda: m.decode(z, out=img2.view))
    B.assert_guards(img2, f"{c['id']} image, traced")
    assert torch.equal(got, plain)
    m._trace = []
    try:
        assert torch.equal(u8_run(), plain_u8) and len(m._trace) == len(recs2)
        assert torch.equal(m.decode_u8(z).cpu(), plain_u8) and len(m._trace) == 2 * len(recs2)
    finally:
        m._trace = None
    m._check_input(z)
    records, rows = traced(m, lambda: m._rows(z))
    assert len(records) == len(recs2) and list(m.state_dict().keys()) == list(P.keys())
    check_trace(c, m, P, records, [z], rows)


def test_the_trace_cannot_be_set_while_the_stream_is_capturing(sfv):
    m = sfv.LDMEncoder(compute_dtype="bf16").cuda()
    x = torch.zeros(8, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = x + 1
        with pytest.raises(RuntimeError):
            m._trace = []
    assert m._trace is None
    m._trace = []                       # outside a capture it can
    m._trace = None


def test_a_graph_encoder_with_a_trace_runs_eager_and_equal(sfv):
    """use_graph=True: with a trace the pass is eager (and recorded); without one the replays give the same bits"""
    c = T.ENC_CASES[0]
    torch.manual_seed(11)
    m = sfv.LDMEncoder(compute_dtype="bf16", use_graph=True).cuda()
    x = T.make_input(c).cuda()
    outs = [m.encode(x, sample=False).clone() for _ in range(3)]
    assert len(m._graphs) == 1
    records, got = traced(m, lambda: m.encode(x, sample=False))
    assert len(records) == len(T.expected_stages(m, c["N"], c["H"], c["W"]))
    assert all(torch.equal(o, got) for o in outs)
