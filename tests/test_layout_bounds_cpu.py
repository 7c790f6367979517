"""The error model of tests/_layout_cases.py without a device: an f32 emulation of every operation passes every bound on every
case (worst |err| / bound printed per quantity), the summands are large enough that one dropped, doubled or misplaced term is 8
bounds away, the tables reach every branch of the restated dispatch, the restated job_blocks_of gives the literal workgroup
counts worked out by hand below, and each of the 23 named defects, injected into an emulation, fails at least one case."""
import numpy as np
import pytest
import torch

import _layout_cases as C
import rbvae_oracle as O

F32_T, BF16_T = C.F32_T, C.BF16_T


# ---- one runner per family: (quantity, case id, thunk -> worst ratio) ------------------------------------------------------------------

def fam_pack(defect=None):
    for c in C.PACK_CASES:
        for dt in (F32_T, BF16_T):
            x = C.pack_data(c)
            yield "pack3", f"{c['id']}-{C.DTN[dt]}", lambda c=c, x=x, dt=dt: C.check_pack(c, x, dt, C.emu_pack(c, x, dt, defect), c["id"])


def fam_permute(defect=None):
    for c in C.PERMUTE_CASES:
        d = C.reduce_data(c)
        yield "permute_reduce", c["id"], lambda c=c, d=d: C.check_sum(C.emu_reduce(c, d, defect), C.reduce_model(c, d), c["id"])


def fam_castpad(defect=None):
    for c in C.CASTPAD_CASES:
        x = C.castpad_data(c)
        yield "cast_pad", c["id"], lambda c=c, x=x: C.check_castpad(c, x, C.emu_castpad(c, x, defect), c["id"])


def _partial(c, d, defect):
    ws = C.emu_colsum_partial(c, d[0], defect)
    C.check_written(ws, torch.ones(ws.shape, dtype=torch.bool), c["id"])
    return C.check_sum(ws, C.partial_model(c, d[0]), c["id"] + " partial", ("block", "column"))


def fam_colsum(defect=None):
    for c in C.COLSUM_CASES:
        d = C.colsum_data(c)
        yield "colsum", c["id"], lambda c=c, d=d: C.check_sum(C.emu_colsum(c, d, defect), C.colsum_model(c, d), c["id"])
        yield "colsum_partial", c["id"], lambda c=c, d=d: _partial(c, d, defect)
    for c in C.REDUCE_ROWS_CASES:
        d = C.reduce_rows_data(c)
        yield "reduce_rows", c["id"], lambda c=c, d=d: C.check_sum(C.emu_final(d[0], c["scale"], d[1], defect), C.reduce_rows_model(c, d), c["id"])


def fam_rows2(defect=None):
    for c in C.ROWS2_CASES:
        d = C.rows2_data(c)
        yield "kind2", c["id"], lambda c=c, d=d: C.check_sum(C.emu_rows2(c, d, defect), C.rows2_model(c, d), c["id"])


def fam_convpack(defect=None):
    for c in C.CONVPACK_CASES:
        x = C.convpack_data(c)
        yield "kind3", c["id"], lambda c=c, x=x: C.check_convpack(c, x, *C.emu_convpack(c, x, defect), c["id"])


def fam_convred(defect=None):
    for c in C.CONVRED_CASES:
        d = C.reduce_data(c)
        yield "kind4", c["id"], lambda c=c, d=d: C.check_sum(C.emu_convred(c, d, defect), C.reduce_model(c, d), c["id"])


def fam_gather(defect=None):
    for c in C.GATHER_CASES:
        d = C.gather_data(c)
        yield "gather", c["id"], lambda c=c, d=d: C.check_gather(c, d, C.emu_gather(c, d, defect), c["id"])


def fam_skinny(defect=None):
    for c in C.SKINNY_CASES:
        d = C.skinny_data(c)
        yield "skinny", c["id"], lambda c=c, d=d: C.check_skinny(c, d, C.emu_skinny(c, d, defect), c["id"])


def fam_vote(defect=None):
    for c in C.VOTE_CASES:
        d = C.vote_data(c)
        yield "state_vote", c["id"], lambda c=c, d=d: C.check_vote(c, d, C.emu_vote(c, d, defect), c["id"])


FAMILIES = [fam_pack, fam_permute, fam_castpad, fam_colsum, fam_rows2, fam_convpack, fam_convred, fam_gather, fam_skinny, fam_vote]


def test_every_emulation_passes_every_bound():
    worst = {}
    for fam in FAMILIES:
        for q, cid, thunk in fam():
            worst[q] = max(worst.get(q, 0.0), thunk())
    print("\nBOUNDS layout emulations worst |err|/bound = " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert set(worst) == {"pack3", "permute_reduce", "cast_pad", "colsum", "colsum_partial", "reduce_rows", "kind2", "kind3", "kind4",
                          "gather", "skinny", "state_vote"}
    for q in ("permute_reduce", "colsum", "colsum_partial", "reduce_rows", "kind2", "kind4", "skinny"):
        assert 0.0 < worst[q] <= 1.0, (q, worst[q])           # the bounds are reached by rounding, not vacuous


def test_no_stored_special_looks_unwritten():
    """The NaN inputs keep a payload whose stored form is not the sentinel of either type."""
    for dt in (F32_T, BF16_T):
        assert not bool(C.is_sentinel(C.store(C.SPECIALS, dt)).any())
    assert int(torch.isnan(C.SPECIALS).sum()) == 2 and int(torch.isinf(C.SPECIALS).sum()) == 2
    up = C.SPECIALS[5:7].to(torch.bfloat16).float()
    assert up.tolist() == [1.0, -2.0]                          # rounded up into the next binade


def sum_models():
    for c in C.PERMUTE_CASES + C.CONVRED_CASES:
        yield c["id"], C.reduce_model(c, C.reduce_data(c))
    for c in C.COLSUM_CASES:
        d = C.colsum_data(c)
        yield c["id"], C.colsum_model(c, d)
        yield c["id"] + " partial", C.partial_model(c, d[0])
    for c in C.REDUCE_ROWS_CASES:
        yield c["id"], C.reduce_rows_model(c, C.reduce_rows_data(c))
    for c in C.ROWS2_CASES:
        yield c["id"], C.rows2_model(c, C.rows2_data(c))


def test_one_term_is_eight_bounds_away():
    n, tight = 0, float("inf")
    for cid, m in sum_models():
        assert float(m["minterm"].min()) >= 0.5 * min(1.0, 0.5)               # |v| >= 0.5, |scale| >= 0.5
        margin = (m["minterm"] / m["bnd"]).min()
        assert margin >= 8, f"{cid}: the smallest term is only {float(margin):.3g} bounds"
        n, tight = n + 1, min(tight, float(margin))
    print(f"\nBOUNDS layout input condition: {n} sum cases, smallest min|term| |scale| / bound = {tight:.3g}")
    assert n > 100


def test_tables_reach_every_branch():
    got = C.covered_branches()
    assert got == set(C.LAYOUT_BRANCHES), (sorted(set(C.LAYOUT_BRANCHES) - got), sorted(got - set(C.LAYOUT_BRANCHES)))
    assert len(C.LAYOUT_BRANCHES) == len(set(C.LAYOUT_BRANCHES))
    # the boundaries the issue names, through the restatements
    assert [C.colsum_rpb(P) for P in (1, 16, 4096, 4097, 8192, 8193)] == [16, 16, 16, 32, 32, 48]
    assert C.colsum_nblk(4097) == 129 and C.colsum_ws_floats(4097, 260) == 129 * 260
    assert [C.gather_gx(fe) for fe in (4, 1200, 4096, 16384)] == [1, 1, 4, 8]
    assert [C.conv_pack_pieces(8, ci, kk, dt)[1:] for ci, kk, dt in ((128, 9, F32_T), (328, 9, BF16_T), (160, 16, BF16_T), (256, 9, BF16_T))] == \
        [(64, 2), (256, 2), (144, 2), (64, 4)]
    vec = {c["id"]: C.colsum_vec(c) for c in C.COLSUM_CASES}
    assert all(v == k.startswith("vec-") for k, v in vec.items()), vec
    wide = {c["id"]: C.rows2_wide(c) for c in C.ROWS2_CASES}
    assert wide == {c["id"]: c["nslab"] >= 1024 and c["n"] in (4, 8, 64) and c["slab"] % 4 == 0 and not c["soff"] for c in C.ROWS2_CASES}
    assert sum(wide.values()) == 5 and sum(1 for c in C.ROWS2_CASES if c["nslab"] == 1024 and not wide[c["id"]]) == 3


def test_job_blocks_of_literals():
    """One row of each kind, the counts by hand from run_jobs_k's loop bounds."""
    rows = [
        C.job_row(0, 0, 0, (5, 7, 9), (63, 1, 7)),                        # 315 elements, a thread each: 2
        C.job_row(0, 0, 0, (5, 64, 9), (576, 1, 64)),                     # inner: 320 (i0, i1) rows: 2
        C.job_row(1, 0, 0, (9, 10, 5), (5, 45, 1), nslab=3, slab=450),    # 450: 2
        C.job_row(2, 0, 0, (1, 1, 64), (0, 0, 1), nslab=2049, slab=64),   # four outputs per workgroup: 16
        C.job_row(2, 0, 0, (1, 1, 5), (0, 0, 1), nslab=63, slab=8),       # 2
        C.job_row(3, 0, 0, (8, 328, 9), dtype=BF16_T),                    # 1 group of 8 channels x 2 pieces (256 + 72): 2
        C.job_row(3, 0, 0, (4, 128, 9), dtype=F32_T),                     # 1 group of 4 x 2 pieces of 64: 2
        C.job_row(3, 0, 0, (5, 6, 9), dtype=F32_T),                       # 2 groups x 1
        C.job_row(4, 0, 0, (3, 520, 9), nslab=2, slab=14040),             # 3 channels x 3 blocks of <= 256: 9
        C.job_row(5, 0, 0, (3, 5, 1024), (0, 0, 5)),                      # a workgroup per row: 3
        [7, 0, 0, 1000, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],              # 4
    ]
    assert [C.job_blocks_of(r) for r in rows] == [2, 2, 2, 16, 2, 2, 2, 2, 9, 3, 4]
    assert [r[14] for r in rows[:3]] == [0, 1, 0] and [r[13] >> 32 for r in rows[:3]] == [1, 1, 2]
    m = C.block_map(rows, 3)
    assert len(m) == 2 + 2 + 2 + 3 + 2 + 2 + 2 + 2 + 3 + 3 + 3
    assert m[6:9] == [[3, 0, 3, 0], [3, 1, 3, 0], [3, 2, 3, 0]]
    assert C.block_map(rows, 65535)[-1] == [10, 3, 4, 0]
    # kind 6: [6, src, dst, d0, d1, d2, first copy's strides x 3, second copy's strides 0 and 1, t1 | t2 << 8, its stride 2, 0, ctx, dst2]
    adam = [
        # tiled (1 802 240 >= 2^20 elements), copies contiguous in i1 (fA = 1) and in i0 (fB = 0): "different", tiles of
        # T0 x T1 x T2 = 32 x 16 x 16 -> 32/32 x 256/16 x ceil(220/16) = 1 x 16 x 14 = 224
        [6, 0, 16, 32, 256, 220, 56320, 1, 256, 1, 32, 1, 8192, 0, 64, 32],
        # tiled (1 106 263 elements), one copy contiguous in i0: 32 x 8 x 32 cut to 32 x 8 x 29 -> ceil(1031/32) x ceil(37/8) x 1
        # = 33 x 5 x 1 = 165
        [6, 0, 16, 1031, 37, 29, 1, 1031, 38147, 0, 0, 1, 0, 0, 64, 0],
        # the same tensor with both copies contiguous in i2 (fA = fB = 2): flat, ceil(1 106 263 / 256) = 4322 (4321 x 256 = 1 106 176)
        [6, 0, 16, 1031, 37, 29, 1073, 29, 1, 29, 29899, 1 | (0 << 8), 1, 0, 64, 32],
        # flat, fewer than 2^20 elements whatever the strides: 64 x 9 x 16 = 9216 = 36 x 256
        [6, 0, 16, 64, 9, 16, 1, 64, 576, 0, 0, 1, 0, 0, 64, 0],
        [6, 0, 16, 5, 7, 3, 1, 5, 35, 0, 0, 0, 0, 0, 64, 0],                # 105 elements: 1
    ]
    assert [C.job_blocks_of(r) for r in adam] == [224, 165, 4322, 36, 1]
    assert [C.job_branch(r) for r in adam] == ["run_jobs_k[6,tiled,different]", "run_jobs_k[6,tiled,one]", "run_jobs_k[6,flat,2]",
                                               "run_jobs_k[6,flat,1]", "run_jobs_k[6,flat,1]"]
    assert [len(C.block_map([r], 256)) for r in adam] == [224, 165, 256, 36, 1]


def test_vote_reference_is_the_oracle():
    for c in C.VOTE_CASES:
        d = C.vote_data(c)
        ref = C.vote_ref(c, d)
        with np.errstate(invalid="ignore"):
            bits = (d[0].numpy() > 0.5).astype(np.float32)
        avg, pct = O.state_consistency(bits, d[1].numpy(), c["n_states"])
        mine = C.vote_consistency(c, ref["out"])
        assert mine[1] == pytest.approx(pct, abs=1e-12) and mine[0] == pytest.approx(avg, abs=1e-12), c["id"]
        _, pat = C.B.SENTINEL[torch.float32]
        assert not (ref["keys"] == pat).any()                    # a key word never looks like an unwritten one
    tie = next(c for c in C.VOTE_CASES if c["special"] == "tie")
    ref = C.vote_ref(tie, C.vote_data(tie))
    assert ref["out"][0].tolist() == [3, 6] and not ref["winners"][0][0]      # two codes with 3 frames each: element 0 = 0 wins
    empty = next(c for c in C.VOTE_CASES if c["special"] == "empty-state")
    assert C.vote_ref(empty, C.vote_data(empty))["out"][2].tolist() == [0, 0]


DEFECTS = {
    "pack_strides_swapped": [fam_pack], "bf16_truncates": [fam_pack, fam_castpad, fam_convpack], "drop_last_slab": [fam_permute],
    "accumulate_ignored": [fam_permute, fam_colsum, fam_rows2, fam_convred], "cast_pad_no_select": [fam_castpad],
    "colsum_drops_short_block": [fam_colsum], "vec_drops_row_tail": [fam_colsum], "vec_skips_ragged_group": [fam_colsum],
    "final_drops_row_tail": [fam_colsum], "wide_drops_tail": [fam_rows2], "dst2_in_dst_order": [fam_convpack],
    "pack_loses_ci0": [fam_convpack], "reduce_doubles_a_slab": [fam_convred], "reduce_loses_ci0": [fam_convred],
    "gather_ignores_counter": [fam_gather], "gather_follows_bad_plan": [fam_gather], "skinny_drops_k_tail": [fam_skinny],
    "skinny_bias_in_every_part": [fam_skinny], "skinny_writes_clamped_rows": [fam_skinny], "vote_ties_to_largest": [fam_vote],
    "vote_lsb_first": [fam_vote], "vote_ge_half": [fam_vote], "vote_counts_across_states": [fam_vote],
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_named_defect_is_rejected(defect):
    assert len(DEFECTS) == 23
    for fam in DEFECTS[defect]:
        failed = []
        for q, cid, thunk in fam(defect):
            if q == "pack3" and "grid-stride" in cid:
                continue                                         # a million elements: the small cases see these defects
            try:
                thunk()
            except AssertionError:
                failed.append(f"{q} {cid}")
        assert failed, f"{defect}: no case of {fam.__name__} noticed"
        print(f"\n{defect}: rejected by {len(failed)} cases of {fam.__name__}, e.g. {failed[0]}")
