"""CPU checks of tests/_ldm_trace_ref.py, the launch-by-launch references of the LDM encoder / decoder trace.

  the restatement IS the reference   with no rounding, the per-op references composed along expected_stages (statistics taken
                                     from the recorded partials, as the device hands them on) equal ldm_oracle.encoder_moments /
                                     _ldm_decoder_ref.decode in float64 within 1e-12 of the largest output, on every case
  the gates are satisfiable          with the storage model as the device, gate (a) (element-wise bound) and gate (b)
                                     (relative L2 <= 2 x the storage model's own) pass on every record of the two 64 x 64
                                     bf16 encoder cases and of the 8 x 8 bf16 decoder case; the floors are printed
  the gates are not slack            each named defect, injected at one record of such a trace, fails gate (a) or (b) AT that
                                     record; the records before it are the clean trace's, which passed: it fails at no earlier
                                     one.  The table is printed (DEFECT ...)
  expected_stages                    on CPU-constructed models with the dispatch queries stubbed both ways it lists every
                                     plan entry exactly once, in plan order, and every case reaches what its row names."""
import functools

import pytest
import torch

import ldm_oracle as LO
import _ldm_decoder_ref as DR
import _ldm_trace_ref as T

ids = lambda cases: [c["id"] for c in cases]
by_id = lambda i: next(c for c in T.ENC_CASES + T.DEC_CASES if c["id"] == i)


@pytest.fixture(scope="module")
def sfv():
    import sfv_amd
    return sfv_amd


@pytest.mark.parametrize("c", T.ENC_CASES + T.DEC_CASES, ids=ids(T.ENC_CASES + T.DEC_CASES))
def test_exact_composition_is_the_reference(sfv, c):
    m, P = T.make_model(sfv, c)
    x = T.make_input(c)
    N, H, W = c["N"], c["H"], c["W"]
    stages = T.expected_stages(m, N, H, W)
    T.assert_reach(c, stages)
    records, last = T.run(m, P, x, "exact")
    assert [(r[0], r[1]) for r in records] == stages
    P64 = {k: v.double() for k, v in P.items()}
    if "forms" in c:
        ref = DR.decode(P64, x.double())
        got = last[:, :3].reshape(N, 8 * H, 8 * W, 3).permute(0, 3, 1, 2)
        assert bool((last[:, 3:] == 0).all())
    else:
        ref = LO.encoder_moments(P64, x.double())
        got = last[:, :8].reshape(N, H // 8, W // 8, 8).permute(0, 3, 1, 2)
    rel = float((got - ref).abs().max() / ref.abs().max())
    print(f"\nEXACT ldm-trace {c['id']}: {len(stages)} records, max |composition - reference| / max |reference| = {rel:.3g}")
    assert rel < 1e-12


MODEL_CASES = ("bf16_halo_2x64x64", "bf16_gather_1x64x64", "bf16_halo_2x8x8")


@functools.lru_cache(maxsize=None)
def model_trace(cid):
    """(parameters, records) of the storage model of a case, every record checked: computed once and shared"""
    import sfv_amd
    c = by_id(cid)
    m, P = T.make_model(sfv_amd, c)
    records, _ = T.run(m, P, T.make_input(c), "model")
    results = [T.check_record(r, P, T.TDT[c["dtype"]]) for r in records]
    return P, records, results


@pytest.mark.parametrize("cid", MODEL_CASES)
def test_storage_model_passes_both_gates(cid):
    P, records, results = model_trace(cid)
    floors = {}
    for r, o in zip(records, results):
        assert o["worst"] <= 1.0
        if o["floor"] is not None:
            assert o["l2"] <= 2 * o["floor"]
            floors.setdefault(r[1], []).append(o["floor"])
    for op, f in floors.items():
        print(f"\nFLOOR ldm-trace {cid} {op}: {len(f)} records, relative L2 of the storage model {min(f):.3g} .. {max(f):.3g}")
    # the rounding of a bf16 store alone is 2^-9 / sqrt(3) = 1.1e-3 for a uniform mantissa; no floor is below a rounding
    assert all(8e-4 < x < 5e-3 for f in floors.values() for x in f)


E0 = "encoder.down.0.block."
DEFECTS = [
    ("dropped_skip", "bf16_halo_2x64x64", (E0 + "1.conv2", "conv3_halo")),
    ("dropped_skip", "bf16_gather_1x64x64", (E0 + "1.conv2", "conv3")),
    ("dropped_skip", "bf16_halo_2x64x64", ("encoder.mid.attn_1.proj_out", "conv1")),
    ("skip_from_h1", "bf16_halo_2x64x64", (E0 + "1.conv2", "conv3_halo")),
    ("skip_from_h1", "bf16_gather_1x64x64", ("encoder.down.2.block.1.conv2", "conv3")),
    ("norm2_with_norm1_statistics", "bf16_halo_2x64x64", (E0 + "1.norm2", "gn_finish")),
    ("statistics_2_percent", "bf16_halo_2x64x64", (E0 + "0.norm1", "gn_finish")),             # conv_in's 8 x 16 tiles
    ("statistics_2_percent", "bf16_halo_2x64x64", (E0 + "1.norm2", "gn_finish")),             # the halo kernel's 16 x 16
    ("statistics_2_percent", "bf16_halo_2x64x64", ("encoder.down.2.block.1.norm1", "gn_finish_ms")),
    ("pad_top_left", "bf16_halo_2x64x64", ("encoder.down.0.downsample.conv", "down")),
    ("pad_top_left", "bf16_gather_1x64x64", ("encoder.down.2.downsample.conv", "down")),
    ("q_k_exchanged", "bf16_halo_2x64x64", ("encoder.mid.attn_1.qkv", "conv1")),
    ("quant_reads_unpadded", "bf16_halo_2x64x64", ("quant_conv", "conv1")),
] + [(d, "bf16_halo_2x8x8", (f"decoder.up.{lvl}.upsample.conv", "up_halo")) for d in T.UP_DEFECTS for lvl in (3, 1)]


@pytest.mark.parametrize("defect,cid,at", DEFECTS, ids=[f"{d}-{c}-{a[0]}" for d, c, a in DEFECTS])
def test_each_named_defect_fails_at_its_record(defect, cid, at):
    P, records, results = model_trace(cid)
    tdt = T.TDT[by_id(cid)["dtype"]]
    i, bad = T.inject(records, P, tdt, defect, at)
    assert all(o["worst"] <= 1.0 for o in results[:i])          # the records before it: the clean trace's
    with pytest.raises(AssertionError) as e:
        T.check_record(bad, P, tdt)
    gate = "b (relative L2)" if "relative L2" in str(e.value) else "a (element-wise)"
    print(f"\nDEFECT ldm-trace {defect} in {cid}: record {i} {at[0]} {at[1]} fails gate {gate}; records 0..{i - 1} pass")
    assert {d for d, _, _ in DEFECTS} == set(T.WIRING_DEFECTS)


def test_a_two_percent_scale_the_statistics_record_cannot_see_fails_the_l2_gate():
    """The convolution normalising with scale / shift 2 % off the recorded ones (the recorded statistics are right, the
    staging reads others): element-wise it is borderline, gate (b) sees it."""
    P, records, results = model_trace("bf16_halo_2x64x64")
    i = next(i for i, r in enumerate(records) if (r[0], r[1]) == (E0 + "1.conv1", "conv3_halo"))
    prefix, op, (x, sc, sh, addend), _, g = records[i]
    M = T.Mode(torch.bfloat16)
    gamma, beta = T.wb(P, g["norm"])
    sc2 = sc * 1.02
    sh2 = beta[None] - (beta[None] - sh) * 1.02               # beta - mean (1.02 scale)
    out = T.evaluate((prefix, op, (x, sc2, sh2, addend), None, g), P, M).model
    bad = (prefix, op, (x, sc, sh, addend), (out[0].bfloat16(), out[1].float()), g)
    with pytest.raises(AssertionError):
        T.check_record(bad, P, torch.bfloat16)
    ref = T.evaluate(records[i], P, M)
    l2 = float((out[0] - ref.ref[0]).norm() / ref.ref[0].norm())
    print(f"\nDEFECT ldm-trace scale 2 % inside {prefix}: relative L2 {l2:.3g} = {l2 / results[i]['floor']:.2f} x the floor")
    assert l2 > 2 * results[i]["floor"]


def _stub(answer):
    return lambda name, *args: answer


@pytest.mark.parametrize("answer", [0, 1])
@pytest.mark.parametrize("c", T.ENC_CASES + T.DEC_CASES, ids=ids(T.ENC_CASES + T.DEC_CASES))
def test_expected_stages_lists_every_plan_entry_once(sfv, c, answer):
    m, _ = T.make_model(sfv, c)
    stages = T.expected_stages(m, c["N"], c["H"], c["W"], query=_stub(answer))
    owner = []
    for prefix, op in stages:
        mine = [i for i, (p, *_) in enumerate(m.plan) if prefix == p or prefix.startswith(p + ".")]
        if prefix == "latent":
            continue
        assert len(mine) == 1, (prefix, op)
        owner.append(mine[0])
    runs = [o for i, o in enumerate(owner) if i == 0 or owner[i - 1] != o]
    assert runs == list(range(len(m.plan))), "a plan entry is missing, repeated or out of order"
    ops = {op for _, op in stages}
    if answer == 0:
        assert not ops & {"conv3_halo", "conv_in", "attention", "up_halo"}
    elif c["impl"] != "gather" or "forms" in c:
        assert "conv3_halo" in ops


def test_the_trace_is_no_state_and_off_by_default(sfv):
    m = sfv.LDMEncoder(compute_dtype="bf16")
    keys = list(m.state_dict().keys())
    assert m._trace is None
    m._trace = []
    assert m._trace == [] and list(m.state_dict().keys()) == keys and not any("trace" in k for k in keys)
    assert not any("trace" in n for n, _ in m.named_buffers())
    m._trace = None
    assert m._trace is None and sfv.LDMDecoder()._trace is None
