"""CPU checks of the keyed dropout restatement (_ends_cases.keyed_keep_mask) and of the case tables of
test_dropout_keyed_gpu.py (tests/_dropout_cases.py): the restatement against a plain Python-int evaluation of
csrc/common.h, its default against what it returned before it took `ec` and `rows`, the drop rate of every p of the GPU
table, the tables against the restated dispatch (every reachable instance, ldo > Nout everywhere), and every named defect
visible on every GPU case it can apply to."""
import hashlib
import struct

import numpy as np
import pytest

import _conv_cases as C
import _dropout_cases as D
import _ends_cases as E
import _halo_cases as H

M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def plain_keep(row, col, Nout, seed, p, seed_dev=None, ec=8):
    """One element's decision in plain Python ints, line by line from csrc/common.h."""
    if seed_dev is not None:
        seed = (seed + seed_dev * 0x9E3779B97F4A7C15) & M64                    # the epilogues' drop_key argument
    x = (seed * 0x9E3779B97F4A7C15 + 0xD6E8FEB86659FD93) & M64                 # drop_key
    x ^= x >> 32
    x = (x * 0xD6E8FEB86659FD93) & M64
    x ^= x >> 32
    k0, k1 = x & M32, x >> 32
    e = col % ec
    idx = row * Nout + col - e                                                 # the chunk's first element
    assert idx <= M64
    run = ((idx & M32) + k0 + (idx >> 32) * k1) & M32                          # drop_run
    s = run                                                                    # drop_bits(run, 0)
    s ^= s >> 16
    s = (s * 0x7feb352d) & M32
    s ^= s >> 15
    s = (s * 0x846ca68b) & M32
    s ^= s >> 16
    for _ in range(e // 2):                                                    # the walk: one xorshift32 step per pair
        s ^= (s << 13) & M32
        s ^= s >> 17
        s ^= (s << 5) & M32
    bits = s >> 16 if e & 1 else s & 0xffff
    pf = struct.unpack("f", struct.pack("f", p))[0]                            # drop_p is a float in the ABI
    thresh16 = int(pf * 4294967296.0) >> 16                                    # (unsigned)((double)drop_p * 2^32) >> 16
    return bits >= thresh16


@pytest.mark.parametrize("ec", [8, 4])
def test_restatement_is_the_hash_by_hand(ec):
    """drop_key, drop_run, drop_bits, the walk and thresh16 in Python ints against the numpy restatement, on rows whose
    element indices lie below, across and far above 2^32: the (idx >> 32) * k1 term of drop_run.  No GPU case reaches that
    term (it needs an output of 8 GB or more), so this host check is all that pins it."""
    Nout = 136
    rows = [0, 1, 127, 128, 31580000, 31580700, 1 << 31, (1 << 33) + 5, 10 ** 12, (1 << 56) + 3]
    assert rows[4] * Nout < 1 << 32 <= rows[5] * Nout
    for seed, seed_dev, p in ((11, None, 0.2), ((1 << 63) | 12345, (1 << 40) + 1, 0.1), (M64, 3, 0.5), (0, 0, 2.0 ** -16),
                              (77, 0x123456789, 65535 / 65536)):
        got = E.keyed_keep_mask(len(rows), Nout, seed, p, seed_dev=seed_dev, ec=ec, rows=rows)
        want = np.array([[plain_keep(r, c, Nout, seed, p, seed_dev, ec) for c in range(Nout)] for r in rows])
        assert np.array_equal(got, want), (seed, seed_dev, p)
        if p in (0.2, 0.1, 0.5):
            assert 0 < int((~want).sum()) < want.size
    # rows= is the same function: row i of the mask is output row rows[i]
    full = E.keyed_keep_mask(300, Nout, 11, 0.2, ec=ec)
    pick = np.array([299, 0, 128, 7])
    assert np.array_equal(E.keyed_keep_mask(4, Nout, 11, 0.2, ec=ec, rows=pick), full[pick])
    assert np.array_equal(full, np.array([[plain_keep(r, c, Nout, 11, 0.2, None, ec) for c in range(Nout)] for r in range(300)]))
    # ec = 4 needs only Nout % 4 == 0, and is another mask than ec = 8
    assert E.keyed_keep_mask(9, 20, 5, 0.2, ec=4).shape == (9, 20)
    assert not np.array_equal(E.keyed_keep_mask(300, Nout, 11, 0.2, ec=4), E.keyed_keep_mask(300, Nout, 11, 0.2, ec=8))
    with pytest.raises(AssertionError):
        E.keyed_keep_mask(9, 20, 5, 0.2, ec=8)


def test_default_is_what_the_function_returned_before():
    """ec = 8 without rows on the arguments of every caller the function had (test_kernels_gpu.py, test_ends_bounds_cpu.py,
    test_gather_deep_ring_gpu.py, cf_build / cf_forward of every CF case with dropout): the digest of those 18 masks, taken
    from the function as it stood before it took `ec` and `rows`."""
    calls = [((777, 136, 11, 0.2), {}), ((999, 136, 11, 0.2), {}), ((999, 136, 11, 0.2), dict(row_stride=144)),
             ((999, 136, 11, 0.2), dict(seed_dev=5)), ((50, 64, 3, 0.0), {}), ((576, 72, 11, 0.2), {})]
    for c in E.CF_CASES:
        if c["drop"]:
            OH, OW = E.s2_out(c["IH"], c["IW"])
            a = (c["N"] * OH * OW, c["Nout"], c["seed"], c["p"], c["seed_dev"])
            calls += [(a, {}), (a, dict(row_stride=c["ldo"]))]
    assert len(calls) == 18
    h = hashlib.sha256()
    for a, k in calls:
        h.update(np.packbits(E.keyed_keep_mask(*a, **k)).tobytes())
        assert np.array_equal(E.keyed_keep_mask(*a, **k), E.keyed_keep_mask(*a, ec=8, rows=np.arange(a[0]), **k))
    assert h.hexdigest() == "fb870d194f95b733690c99c477ceec64775ad9413a7dad1b7ef08944e517e361"


@pytest.mark.parametrize("ec", [8, 4])
@pytest.mark.parametrize("p", D.P_TABLE)
def test_drop_rate_of_every_p_of_the_gpu_table(p, ec):
    """Within 5 sigma of thresh16 / 65536 over 2^20 elements (exactly none at p = 0)."""
    q = D.thresh16(p) / 65536.0
    keep = E.keyed_keep_mask(4096, 256, D.seed_of(f"rate{p}{ec}"), p, ec=ec)
    n = keep.size
    dropped = n - int(keep.sum())
    assert abs(dropped - n * q) <= 5 * (n * q * (1 - q)) ** 0.5, (p, ec, dropped, n * q)
    assert {D.thresh16(x) for x in D.P_EDGE} == {0, 1, 6553, 32768, 0xFFFF} and D.thresh16(D.P_MAIN) == 13107


def cs_width(d):
    """cs_bn (csrc/conv_s2.hip): output channels per workgroup."""
    return 256 if d["Nout"] % 256 == 0 else 128


def test_tables_reach_every_instance_and_every_case_has_a_padded_pitch():
    for d in D.GG_DROP:
        assert C.gg_case_instance(d["src"])[0] == d["src"]["inst"], d["id"]
    assert {(d["dtype"], d["src"]["inst"]) for d in D.GG_DROP} == C.GG_REACHABLE
    # the two large cases stay: nothing else reaches these two f32 branches
    assert [d["id"] for d in D.GG_DROP if (d["dtype"], d["src"]["inst"]) in {("f32", "ns2"), ("f32", "ns1_512")}] == \
        ["ns1_512_f32", "ns2_f32"]
    assert {H.dh_instance(d["src"]) for d in D.DH_DROP} == H.DH_REACHABLE
    for d in D.DH_DROP:
        c = d["src"]
        assert H.dh_tile_rows(c["dtype"], c["N"], c["TH"], c["TW"], c["Kc"], c["Nout"]) in (128, 256)
    assert {cs_width(d) for d in D.CS_DROP} == {128, 256} and any(d["M"] == 1 for d in D.CS_DROP)      # the 2 x 2 image
    assert len(D.BY_ID) == len(D.ALL_DROP) == 22 + 12 + 5
    for d in D.ALL_DROP:
        es = 16 // d["ec"]
        assert d["ldo"] > d["Nout"] and d["ldo"] * es % 16 == 0 and d["Nout"] % d["ec"] == 0, d["id"]
        assert np.array_equal(np.sort(d["rows"]), np.arange(d["M"])), d["id"]            # the classes tile the output
    assert {(D.BY_ID[i]["kind"], D.BY_ID[i]["dtype"]) for i in D.SEED_DEV_IDS} == \
        {("gg", "bf16"), ("gg", "f32"), ("dh", "bf16"), ("dh", "f32"), ("cs", "bf16")}
    assert [(D.BY_ID[i]["kind"], D.BY_ID[i]["dtype"]) for i in D.THRESH_IDS] == \
        [("gg", "bf16"), ("gg", "f32"), ("dh", "bf16"), ("cs", "bf16")]


ROW_DEFECTS = ("pitch_ldo", "tile_local_row", "class_local_row", "ec8_on_f32")


@pytest.mark.parametrize("d", D.ALL_DROP, ids=[d["id"] for d in D.ALL_DROP])
def test_index_defects_change_the_mask_of_every_case(d):
    """The leading dimension as the row pitch, the row inside the tile, the row inside the parity class and the bf16 walk
    on f32 each give another mask on EVERY case they can apply to (on a thinned copy of the case: about 8192 of its rows,
    spread over the classes).  What cannot apply: class rows where there are no classes, the f32 walk on bf16, and any
    row formula on the 2 x 2 image, whose single output row is row 0 under each of them."""
    t = D.thinned(d)
    want = D.keep_mask(t, scatter=False)
    applied = set()
    for defect in ROW_DEFECTS:
        bad = D.keep_mask(t, defect=defect, scatter=False)
        if bad is not None:
            applied.add(defect)
            assert bad.shape == want.shape and not np.array_equal(bad, want), (d["id"], defect)
            assert 0.1 < (bad != want).mean() < 0.5 or d["M"] * d["Nout"] < 4096, (d["id"], defect)     # no near miss
    expect = set()
    if d["M"] > 1:
        expect |= {"pitch_ldo", "tile_local_row"}
    if d["kind"] == "dh" or (d["kind"] == "gg" and d["src"]["op"] == "dgrad"):
        expect.add("class_local_row")
    if d["dtype"] == "f32":
        expect.add("ec8_on_f32")
    assert applied == expect, (d["id"], applied, expect)


def test_thinning_keeps_the_full_mask():
    d = D.BY_ID["n64_bf16"]
    t = D.thinned(d, 500)
    assert np.array_equal(D.keep_mask(t, scatter=False), D.keep_mask(d)[t["rows"]])
    assert d["local"] is not None and len(set(t["rows"] // (2 * 11) % 2)) == 2 and len(set(t["rows"] % 2)) == 2   # all classes


@pytest.mark.parametrize("id", D.SEED_DEV_IDS)
def test_seed_dev_defects_change_the_mask(id):
    d = D.BY_ID[id]
    t = D.thinned(d)
    seed = D.seed_of(id, top=True)
    assert seed >> 63 == 1
    null = D.keep_mask(t, seed=seed, scatter=False)
    seen = [null]
    for v in D.SEED_DEV_VALUES:
        want = D.keep_mask(t, seed=seed, seed_dev=v, scatter=False)
        assert np.array_equal(want, null) == (v == 0), (id, v)
        for defect in ("seed_dev_ignored", "seed_dev_no_gold"):
            bad = D.keep_mask(t, seed=seed, seed_dev=v, defect=defect, scatter=False)
            assert (bad is None) == (v == 0), (id, v, defect)
            if bad is not None:
                assert not np.array_equal(bad, want), (id, v, defect)
        if v:
            assert not any(np.array_equal(want, s) for s in seen), (id, v)
            seen.append(want)


@pytest.mark.parametrize("id", D.THRESH_IDS)
def test_threshold_table_and_the_rounding_defect(id):
    """Every p of the table gives another mask than the one before it (the thresholds are strictly increasing and each
    case is large enough to have elements between two of them), p = 0 keeps everything, and thresh16 = round(p 2^16) shows
    on every threshold case at p = 0.1 -- the one p of the table at which floor and round differ (0, 1, 13107.2, 32768 and
    65535 round to themselves)."""
    t = D.BY_ID[id]                                                      # whole: the edges need every element
    assert 4e5 < t["M"] * t["Nout"] < 2.1e6
    masks = {p: D.keep_mask(t, p=p, scatter=False) for p in D.P_TABLE}
    assert masks[0.0].all()
    ps = sorted(D.P_TABLE)
    for a, b in zip(ps, ps[1:]):
        assert D.thresh16(a) < D.thresh16(b)
        assert not (masks[b] & ~masks[a]).any() and (masks[a] & ~masks[b]).any(), (id, a, b)     # nested, strictly
    assert 0 < masks[ps[-1]].sum() < masks[ps[-1]].size / 1000                                   # a few survivors
    for p in D.P_TABLE:
        bad = D.keep_mask(t, p=p, defect="thresh_rounded", scatter=False)
        assert (bad is not None) == (p == 0.1), (id, p)
        if bad is not None:
            assert not np.array_equal(bad, masks[p]), (id, p)


def test_the_step_wiring_masks_are_pairwise_different():
    """What test_dropout_keyed_gpu.py expects of a trainer step: the four sites' keys (noise_key * 8 + 1 .. 4) and the
    counters 0 .. 2 give twelve different masks on the smallest saved activation (B = 2, T = 3, 32 x 32 frames: 768 rows
    of 256 channels) -- one key for two layers, or a counter that does not advance, repeats one."""
    from importlib import import_module
    key = import_module("symbols-from-video_amd.trainer").noise_key(17, 0)
    masks = [E.keyed_keep_mask(768, 256, key * 8 + k, 0.2, seed_dev=step) for step in range(3) for k in range(1, 5)]
    for i in range(len(masks)):
        for j in range(i):
            assert 0.2 < (masks[i] != masks[j]).mean() < 0.45, (i, j)
