"""The keyed dropout mask (drop_mode 1) of the four epilogues that draw it, element for element and per kernel instance
(test_dropout_keyed_gpu.py / test_dropout_keyed_cpu.py): case tables and the expected mask of every case, optionally under
one named defect.  The hash itself has ONE host definition, _ends_cases.keyed_keep_mask; everything here only chooses its
arguments.

  csrc/gather_gemm.hip   rbvae_gather_gemm: every entry of _conv_cases.GG_CASES by its geometry (shape, Kc, Nout, dtype,
                         op; the column-sum cases keep their colsum_ws, which is part of the dispatch), i.e. every
                         (dtype, branch) of GG_REACHABLE
  csrc/deconv_halo.hip   rbvae_deconv3x3s2_halo: every entry of _halo_cases.DH_CASES in its forward form
  csrc/conv_s2.hip       rbvae_conv3x3s2_halo: the five shapes of test_conv3x3s2_halo_bounded_and_guarded
  (csrc/conv_first.hip   rbvae_conv_first_fused is covered by _ends_cases.CF_CASES, seed_dev included)

A case here is reduced to what the mask depends on: dict(kind, id, dtype, ec, M, Nout, ldo, rows, local, tile_local, seed)
with rows [M] the output row of every (class, m) in class order -- _conv_cases.gg_out_rows for the gather GEMM, dh_out_rows
for the deconvolution's four parity classes, 0 .. M - 1 otherwise -- local [M] the row inside its class (the input-grid row
m) where there are classes, tile_local [M] the row inside its tile.  Every case has ldo > Nout, so that an index built
from the leading dimension shows.

P_MAIN = 0.2 is the engine's dropout rate (scale 1.25 = 1 / (1 - 0.2)); at 0.2 floor(p 2^16) = round(p 2^16), so the
floor / round defect is a matter of the threshold table alone: P_EDGE holds 0.1 for it (6553 against 6554), beside the
edges thresh16 = 0, 1 and 0xFFFF of the packed 16-bit decision and 0.5."""
import numpy as np

import _conv_cases as C
import _halo_cases as H
from _ends_cases import GOLD, keyed_keep_mask

P_MAIN, SCALE = 0.2, 1.25
P_EDGE = (0.0, 2.0 ** -16, 0.1, 0.5, 65535.0 / 65536.0)
P_TABLE = (P_MAIN,) + P_EDGE
SEED_DEV_VALUES = (0, 3, (1 << 40) + 1)
EC = {"bf16": 8, "f32": 4}
M64 = (1 << 64) - 1


def thresh16(p):
    """floor(f32(p) * 2^32) >> 16 (the four host wrappers)."""
    return int(float(np.float32(p)) * 4294967296.0) >> 16


def seed_of(id, top=False):
    """A full-width 64-bit seed per case (top: the top bit set, as the seed_dev cases want it)."""
    s = (sum(map(ord, id)) * GOLD + 0x632BE59BD9B4E019) & M64
    return s | (1 << 63) if top else s


# ---- rbvae_gather_gemm ------------------------------------------------------------------------------------------------------

def gg_drop(c):
    ec, Nout = EC[c["dtype"]], c["Nout"]
    geom, desc, ncls, taps, Mc, rows, nhw, mt = C.gg_geometry(c)
    orow = C.gg_out_rows(c).numpy()                                       # [ncls][Mc]
    m = np.tile(np.arange(Mc), ncls)
    return dict(kind="gg", id=c["id"], src=c, dtype=c["dtype"], ec=ec, M=rows, Nout=Nout, ldo=max(c["ldo"], Nout + ec),
                rows=orow.reshape(-1), local=m if ncls > 1 else None, tile_local=m % 128, seed=seed_of(c["id"]))


GG_DROP = [gg_drop(c) for c in C.GG_CASES]


# ---- rbvae_deconv3x3s2_halo -------------------------------------------------------------------------------------------------

def dh_out_rows(c):
    """Output row of every (class 2 ch + cw, input-grid row m = (n TH + a) TW + b): (n 2TH + 2a + ch) 2TW + 2b + cw."""
    N, TH, TW = c["N"], c["TH"], c["TW"]
    m = np.arange(N * TH * TW)
    n, a, b = m // (TH * TW), m // TW % TH, m % TW
    return np.stack([(n * 2 * TH + 2 * a + ch) * 2 * TW + 2 * b + cw for ch in (0, 1) for cw in (0, 1)])


def dh_drop(c):
    ec, Nout = EC[c["dtype"]], c["Nout"]
    orow = dh_out_rows(c)
    return dict(kind="dh", id=c["id"], src=c, dtype=c["dtype"], ec=ec, M=orow.size, Nout=Nout, ldo=max(c["ldo"], Nout + ec),
                rows=orow.reshape(-1), local=np.tile(np.arange(orow.shape[1]), 4), tile_local=orow.reshape(-1) % 128,
                seed=seed_of(c["id"]))


DH_DROP = [dh_drop(c) for c in H.DH_CASES]


# ---- rbvae_conv3x3s2_halo ---------------------------------------------------------------------------------------------------

CS_SHAPES = [(2, 32, 128, 16, 32), (2, 256, 256, 44, 80), (5, 96, 128, 8, 8), (1, 128, 256, 34, 66), (1, 64, 128, 2, 2)]


def cs_drop(N, Kc, Nout, IH, IW):
    OH, OW = IH // 2, IW // 2
    id = f"cs_{N}x{Kc}x{Nout}x{IH}x{IW}"
    r = np.arange(N * OH * OW)
    return dict(kind="cs", id=id, src=dict(N=N, Kc=Kc, Nout=Nout, IH=IH, IW=IW, lda=Kc + 32), dtype="bf16", ec=8, M=r.size,
                Nout=Nout, ldo=Nout + 8, rows=r, local=None, tile_local=(r // OW % OH % 8) * 16 + r % OW % 16,
                seed=seed_of(id))


CS_DROP = [cs_drop(*s) for s in CS_SHAPES]

ALL_DROP = GG_DROP + DH_DROP + CS_DROP
BY_ID = {d["id"]: d for d in ALL_DROP}

# one case per kernel and dtype for the device step counter; one bf16 and one f32 gather GEMM and one case of each halo
# kernel for the threshold table.  The seed_dev cases are small (each runs four times); the threshold cases have 0.45 to
# 2 M elements, so that thresh16 = 1 drops a few and thresh16 = 0xFFFF keeps a few (7 to 30 expected)
SEED_DEV_IDS = ("n64_bf16", "ns3_64_f32", "bf16_sc4_w4_grad", "f32_sc8_w4_grad", "cs_5x96x128x8x8")
THRESH_IDS = ("ns3_128_bf16", "ns3_256_f32", "bf16_sc16_w4_grad", "cs_2x256x256x44x80")


# ---- the expected mask, and the same under one named defect -----------------------------------------------------------------

DEFECTS = ("pitch_ldo", "tile_local_row", "class_local_row", "ec8_on_f32", "seed_dev_ignored", "seed_dev_no_gold",
           "thresh_rounded")


def thinned(d, n=8192):
    """Case d with about n of its (class, m) entries, evenly spread over the classes: what a defect changes there it changes
    in the whole mask.  For keep_mask(.., scatter=False) only (the entries no longer cover the output)."""
    sel = np.arange(0, d["rows"].size, max(1, d["rows"].size // n))
    pick = lambda a: None if a is None else a[sel]
    return dict(d, M=sel.size, rows=d["rows"][sel], local=pick(d["local"]), tile_local=d["tile_local"][sel], rows_total=d["M"])


def keep_mask(d, p=P_MAIN, seed=None, seed_dev=None, defect=None, scatter=True):
    """Keep-mask [M][Nout] by OUTPUT row of case d (numpy bool; scatter=False: in the case's own (class, m) order), or None
    where `defect` cannot apply to the case:
      pitch_ldo         the index's row pitch is the leading dimension (a single-row output has only row 0: cannot apply)
      tile_local_row    the row inside the tile (row % 128; the 8 x 16 pixel tile of conv_s2) instead of the output row
      class_local_row   the row inside the parity class (the input-grid row) instead of the scattered output row
      ec8_on_f32        the bf16 chunk walk (8 elements per hash) on f32 storage
      seed_dev_ignored  the device step counter is not read (needs seed_dev != 0)
      seed_dev_no_gold  seed + seed_dev without the golden-ratio multiply (needs seed_dev != 0)
      thresh_rounded    thresh16 = round(p 2^16) instead of floor (needs a p at which the two differ)"""
    assert defect is None or defect in DEFECTS
    seed = d["seed"] if seed is None else seed
    rows, ec, stride = d["rows"], d["ec"], None
    if defect == "pitch_ldo":
        if d.get("rows_total", d["M"]) == 1:
            return None
        stride = d["ldo"]
    elif defect == "tile_local_row":
        if np.array_equal(d["tile_local"], rows):
            return None
        rows = d["tile_local"]
    elif defect == "class_local_row":
        if d["local"] is None:
            return None
        rows = d["local"]
    elif defect == "ec8_on_f32":
        if d["dtype"] != "f32":
            return None
        ec = 8
    elif defect in ("seed_dev_ignored", "seed_dev_no_gold"):
        if not seed_dev:
            return None
        seed, seed_dev = ((seed + seed_dev) & M64 if defect == "seed_dev_no_gold" else seed), None
    elif defect == "thresh_rounded":
        t = int(np.floor(float(np.float32(p)) * 65536.0 + 0.5))
        if t == thresh16(p):
            return None
        p = t / 65536.0                                                  # exact in f32: floor(p 2^32) >> 16 = t
    part = keyed_keep_mask(d["M"], d["Nout"], seed, p, seed_dev=seed_dev, row_stride=stride, ec=ec, rows=rows)
    if not scatter:
        return part
    out = np.empty_like(part)
    out[d["rows"]] = part                                                # class order -> output rows
    return out
