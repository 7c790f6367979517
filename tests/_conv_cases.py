"""The gather_gemm / wgrad_gemm cases of test_conv_bounds_gpu.py, the host restatement of the kernels' dispatch that
names the template instance each case reaches, and the float64 operands and references of the cases (CPU only: the
GPU tests upload what is built here, test_bounds_cpu.py checks the table without a GPU)."""
import torch

import _bounds as B

KE = {"f32": 32, "bf16": 64}                   # elements per 128-byte K slice
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
DTYPE_ID = {"f32": 0, "bf16": 1}


def cdiv(a, b):
    return -(-a // b)


def conv_out(n, k=3):
    return (n + 2 - k) // 2 + 1


def conv_classes(k=3):
    """gather_gemm descriptor of Conv2d(k, stride s, pad 1): one class, k*k taps at (kh - 1, kw - 1)."""
    d = [k * k, 0, 0]
    for kh in range(k):
        for kw in range(k):
            d += [kh * k + kw, kh - 1, kw - 1]
    return d, 1


def dgrad_classes(k=3):
    """The four output-parity classes of the stride-2 conv's input gradient, heaviest first (engine.dgrad_classes)."""
    per = []
    for ch in (0, 1):
        for cw in (0, 1):
            taps = []
            for kh in range(k):
                if (ch + 1 - kh) % 2:
                    continue
                for kw in range(k):
                    if (cw + 1 - kw) % 2:
                        continue
                    taps += [kh * k + kw, (ch + 1 - kh) // 2, (cw + 1 - kw) // 2]
            per.append((len(taps) // 3, ch, cw, taps))
    per.sort(key=lambda t: -t[0])
    d = []
    for n, ch, cw, taps in per:
        d += [n, ch, cw] + taps
    return d, len(per)


ONE_TAP = ([1, 0, 0, 0, 0, 0], 1)


def parse_desc(desc, ncls):
    """[(ntaps, oh0, ow0)] per class of a class descriptor."""
    out, i = [], 0
    for _ in range(ncls):
        out.append((desc[i], desc[i + 1], desc[i + 2]))
        i += 3 + 3 * desc[i]
    return out


# ---- gather_gemm ----------------------------------------------------------------------------------------------------

def gg_instance(dtype, Mc, Nout, nclass, max_steps, colsum):
    """dispatch_gg (csrc/gather_gemm.hip) as built: (branch, (NT, WAVES, NS, OCC, BM)) of gather_gemm_k<T, ...>."""
    blocks = cdiv(Mc, 128) * cdiv(Nout, 128 if Nout > 64 else 64) * nclass
    ns = 1 if max_steps <= 2 else (2 if blocks > 256 else 3)
    if ns == 3 and blocks > 128 and max_steps >= 8:
        ns = 4
    bf = dtype == "bf16"
    if Nout <= 64 and blocks <= 128 and max_steps >= 16 and bf and not colsum:
        return "nout64_deep", (2, 4, 3, 1, 64)
    if Nout <= 64:
        return ("nout64_ns1", (2, 4, 1, 1, 128)) if ns == 1 else ("nout64", (2, 4, 2, 1, 128))
    if ns == 3:
        if blocks <= 64 and not colsum and bf:
            return "ns3_64sq", (2, 4, 3, 1, 64)
        if blocks <= 64:
            return "ns3_64", (1, 4, 3, 1, 128)
        if blocks <= 128:
            return "ns3_128", (2, 4, 3, 1, 128)
    if ns == 1 and blocks > 512:
        return "ns1_512", (2, 4, 1, 4, 128)
    if ns == 1:
        return "ns1", (4, 4, 1, 1, 128)
    if ns == 2:
        return "ns2", (4, 8, 2, 1, 128)
    if ns >= 4:
        return "ns4", (4, 8, 4, 1, 128)
    return "ns3_256", (4, 8, 3, 1, 128)


# every (dtype, branch) the build reaches through the public ABI: dispatch_gg reads branch for branch like gg_instance above
# (the 64-row tile is instantiated for bf16 only)
GG_REACHABLE = {("bf16", "nout64_deep")} | {(d, b) for d in ("f32", "bf16") for b in (
    "nout64_ns1", "nout64", "ns3_64", "ns3_128", "ns1_512", "ns1", "ns2", "ns4", "ns3_256")} | {("bf16", "ns3_64sq")}


def gg(id, dtype, op, shape, Kc, Nout, inst, lda=0, ldo=0, **epi):
    """One gather_gemm case: op in linear / conv_s2 / conv_s1 / dgrad; shape = (M,) for linear, (N, H, W) of A's pixel grid
    otherwise; lda / ldo = padding columns; epi: bias, relu, scale, gate, addend, mask, colsum."""
    return dict(id=id, dtype=dtype, op=op, shape=shape, Kc=Kc, Nout=Nout, inst=inst, lda=Kc + lda, ldo=Nout + ldo, epi=epi)


GG_CASES = [
    gg("deep64_bf16", "bf16", "conv_s2", (2, 30, 30), 128, 56, "nout64_deep", lda=64, ldo=8, bias=1, relu=1, scale=0.75),
    gg("deep64_pow2_bf16", "bf16", "conv_s2", (3, 32, 32), 128, 40, "nout64_deep", gate=1),
    gg("n64ns1_f32", "f32", "linear", (1000,), 64, 40, "nout64_ns1", lda=32, ldo=8, bias=1, gate=1),
    gg("n64ns1_bf16", "bf16", "linear", (777,), 128, 64, "nout64_ns1", lda=8, ldo=8, colsum=1, addend=1),
    gg("n64_f32", "f32", "conv_s2", (2, 22, 26), 32, 48, "nout64", colsum=1, mask=1, scale=1.25),
    gg("n64_bf16", "bf16", "dgrad", (2, 9, 11), 64, 24, "nout64", lda=64, ldo=8, bias=1, relu=1),
    gg("ns3sq_bf16", "bf16", "conv_s2", (2, 34, 34), 64, 200, "ns3_64sq", ldo=8, bias=1, relu=1, gate=1),
    gg("ns3_64_f32", "f32", "conv_s1", (1, 20, 20), 64, 72, "ns3_64", lda=32, addend=1, scale=-0.5),
    gg("ns3_64_bf16", "bf16", "dgrad", (2, 9, 9), 64, 136, "ns3_64", colsum=1, bias=1, scale=2.0),
    gg("ns3_128_f32", "f32", "dgrad", (2, 36, 40), 32, 72, "ns3_128", ldo=8, bias=1, colsum=1, gate=1),
    gg("ns3_128_bf16", "bf16", "linear", (8000,), 192, 136, "ns3_128", lda=64, relu=1, mask=1, scale=1.25),
    gg("ns1_512_f32", "f32", "linear", (16500,), 32, 520, "ns1_512", ldo=4, bias=1, colsum=1),
    gg("ns1_512_bf16", "bf16", "linear", (13100,), 64, 520, "ns1_512", lda=64, bias=1, colsum=1, relu=1),
    gg("ns1_f32", "f32", "linear", (300,), 64, 136, "ns1", ldo=8, colsum=1, relu=1, bias=1),
    gg("ns1_bf16", "bf16", "linear", (1300,), 128, 392, "ns1", ldo=8, addend=1, gate=1),
    gg("ns2_f32", "f32", "conv_s2", (4, 130, 130), 32, 136, "ns2", lda=32, bias=1, relu=1, colsum=1),
    gg("ns2_bf16", "bf16", "dgrad", (2, 48, 44), 64, 200, "ns2", ldo=8, gate=1, scale=0.5),
    gg("ns4_f32", "f32", "conv_s1", (3, 56, 56), 32, 136, "ns4", ldo=4, bias=1, addend=1),
    gg("ns4_bf16", "bf16", "conv_s2", (2, 144, 144), 64, 200, "ns4", lda=64, ldo=8, bias=1, relu=1, mask=1, scale=1.25),
    gg("ns4_pow2_bf16", "bf16", "conv_s2", (3, 128, 128), 64, 136, "ns4", colsum=1, bias=1),
    gg("ns3_256_f32", "f32", "linear", (10000,), 128, 200, "ns3_256", lda=32, ldo=8, gate=1, bias=1),
    gg("ns3_256_bf16", "bf16", "dgrad", (3, 30, 30), 64, 136, "ns3_256", ldo=8, bias=1, colsum=1, relu=1),
]


def gg_geometry(c):
    """(geom, desc, ncls, taps_total, Mc, out_rows, out_nhw, max_taps) of a case as rbvae_gather_gemm takes it."""
    op = c["op"]
    if op == "linear":
        M = c["shape"][0]
        return (M, 1, 1, 1, 1, 1, 1, 1, 1), *ONE_TAP, 1, M, M, None, 1
    N, H, W = c["shape"]
    if op == "conv_s2":
        Ho, Wo = conv_out(H), conv_out(W)
        return (N, H, W, Ho, Wo, 2, Ho, Wo, 1), *conv_classes(), 9, N * Ho * Wo, N * Ho * Wo, (N, Ho, Wo), 9
    if op == "conv_s1":
        return (N, H, W, H, W, 1, H, W, 1), *conv_classes(), 9, N * H * W, N * H * W, (N, H, W), 9
    assert op == "dgrad"
    d, n = dgrad_classes()
    return (N, H, W, H, W, 1, 2 * H, 2 * W, 2), d, n, 9, N * H * W, N * 4 * H * W, (N, 2 * H, 2 * W), 4


def gg_case_instance(c):
    geom, desc, ncls, taps, Mc, rows, nhw, mt = gg_geometry(c)
    return gg_instance(c["dtype"], Mc, c["Nout"], ncls, mt * (c["Kc"] // KE[c["dtype"]]), bool(c["epi"].get("colsum")))


def gg_out_rows(c):
    """orow of every (class, m): [ncls][Mc] (the rows a 128-row tile of a class stores, for its column sums)."""
    geom, desc, ncls, taps, Mc, rows, nhw, mt = gg_geometry(c)
    Nimg, IH, IW, TH, TW, sa, OH, OW, so = geom
    m = torch.arange(Mc)
    n, rem = m // (TH * TW), m % (TH * TW)
    a, b = rem // TW, rem % TW
    return torch.stack([(n * OH + a * so + oh0) * OW + b * so + ow0 for _, oh0, ow0 in parse_desc(desc, ncls)])


def gg_build(c):
    """Operands (storage-rounded, CPU) and the float64 reference of a case: dict with A [rows][Kc], Wp [Nout][taps][Kc],
    bias, gate, addend, keep, and ref / S / pre as [out_rows][Nout]."""
    tdt, Kc, Nout, e = TDT[c["dtype"]], c["Kc"], c["Nout"], c["epi"]
    geom, desc, ncls, taps, Mc, rows, nhw, mt = gg_geometry(c)
    g = torch.Generator().manual_seed(sum(map(ord, c["id"])))
    op = c["op"]
    if op == "linear":
        A = torch.randn(c["shape"][0], Kc, generator=g).to(tdt)
        Wt = (torch.randn(Nout, Kc, generator=g) / Kc ** 0.5).to(tdt)
        ref, S = B.ref_and_scale("linear", A, Wt)
        Wp, K = Wt, Kc
    else:
        N, H, W = c["shape"]
        x = torch.randn(N, Kc, H, W, generator=g).to(tdt)
        if op == "dgrad":
            w = (torch.randn(Kc, Nout, 3, 3, generator=g) / (Kc * 4) ** 0.5).to(tdt)     # Conv2d(Nout -> Kc) weight
            ref, S = B.ref_and_scale("conv_transpose2d", x, w)
            Wp = w.permute(1, 2, 3, 0).contiguous()                                      # [ci][kh][kw][co]
            K = 4 * Kc
        else:
            w = (torch.randn(Nout, Kc, 3, 3, generator=g) / (Kc * 9) ** 0.5).to(tdt)
            ref, S = B.ref_and_scale("conv2d", x, w, stride=2 if op == "conv_s2" else 1)
            Wp = w.permute(0, 2, 3, 1).contiguous()                                      # [co][kh][kw][ci]
            K = 9 * Kc
        A = B.rows(x)
        ref, S = B.rows(ref), B.rows(S)
    out = dict(A=A, Wp=Wp.reshape(Nout, -1), K=K, geom=geom, desc=desc, ncls=ncls, taps=taps, Mc=Mc, rows=rows, nhw=nhw,
               bias=None, gate=None, addend=None, keep=None, pre=None, scale=float(e.get("scale", 1.0)))
    assert ref.shape == (rows, Nout)
    if e.get("bias"):
        out["bias"] = torch.randn(Nout, generator=g) * 0.5
        ref = ref + out["bias"].double()
        S = S + out["bias"].double().abs()
    if e.get("relu"):
        ref = ref.clamp_min(0)
    ref = ref * out["scale"]
    if e.get("mask"):
        out["keep"] = torch.rand(rows, Nout, generator=g) > 0.2
        ref = ref * out["keep"]
    if e.get("addend"):
        out["addend"] = torch.randn(rows, Nout, generator=g).to(tdt)
        out["pre"] = ref
        ref = ref + out["addend"].double()
    if e.get("gate"):
        out["gate"] = torch.randn(rows, Nout, generator=g).to(tdt)
        ref = ref * (out["gate"] > 0)
    out["ref"], out["S"] = ref, S
    return out


# ---- wgrad_gemm -----------------------------------------------------------------------------------------------------

def wg_instance(dtype, P, Co, Ci, taps, ksplit):
    """rbvae_wgrad_gemm's choice (csrc/wgrad_gemm.hip, launch_wg / launch_wg_ns) as built: ((T, NT, NS, BM), grid, blocks)."""
    Pper = cdiv(cdiv(P, ksplit), 64) * 64
    NT = 2 if Ci > 64 else 1
    BM = 64 if dtype == "f32" and Co <= 64 else 128
    BK, ES = (64, 2) if dtype == "bf16" else (32, 4)
    blocks = cdiv(Co, BM) * cdiv(Ci, 64 * NT) * taps * ksplit
    lds2 = 2 * BK * (BM + 64 * NT) * ES + Pper * 4
    NS = 2 if blocks > 256 and 2 * lds2 <= 160 * 1024 else 3
    grid = 8 * cdiv(blocks, 8) if ksplit > 1 else blocks
    return (dtype, NT, NS, BM), grid, blocks


WG_REACHABLE = {(d, nt, ns, bm) for d, bm in (("f32", 64), ("f32", 128), ("bf16", 128)) for nt in (1, 2) for ns in (2, 3)}


def wg(id, dtype, op, shape, Co, Ci, ks, inst, ldy=0, ldi=0):
    """One wgrad_gemm case: op conv (3x3 s2 p1 with its gather table; shape = (N, H, W) of the input) or linear
    (no table; shape = (P,))."""
    return dict(id=id, dtype=dtype, op=op, shape=shape, Co=Co, Ci=Ci, ks=ks, inst=inst, ldy=Co + ldy, ldi=Ci + ldi)


WG_CASES = [
    wg("bm64_nt1_ns3_f32", "f32", "conv", (2, 20, 20), 40, 64, 1, ("f32", 1, 3, 64), ldy=8),
    wg("bm64_nt1_ns2_f32", "f32", "conv", (2, 62, 62), 64, 64, 29, ("f32", 1, 2, 64), ldi=8),
    wg("bm64_nt2_ns3_f32", "f32", "conv", (1, 24, 24), 64, 136, 2, ("f32", 2, 3, 64)),
    wg("bm64_nt2_ns2_f32", "f32", "conv", (2, 40, 40), 56, 192, 15, ("f32", 2, 2, 64), ldy=8, ldi=4),
    wg("bm128_nt1_ns3_f32", "f32", "conv", (2, 18, 18), 200, 64, 1, ("f32", 1, 3, 128)),
    wg("bm128_nt1_ns2_f32", "f32", "linear", (8300,), 136, 40, 130, ("f32", 1, 2, 128), ldi=4),
    wg("bm128_nt2_ns3_f32", "f32", "conv", (2, 30, 30), 136, 200, 3, ("f32", 2, 3, 128), ldy=4),
    wg("bm128_nt2_ns2_f32", "f32", "conv", (2, 32, 32), 256, 256, 9, ("f32", 2, 2, 128)),
    wg("nt1_ns3_bf16", "bf16", "conv", (3, 16, 16), 64, 64, 2, ("bf16", 1, 3, 128), ldy=8, ldi=8),
    wg("nt1_ns2_bf16", "bf16", "linear", (4500,), 392, 56, 71, ("bf16", 1, 2, 128), ldi=8),
    wg("nt2_ns3_bf16", "bf16", "conv", (2, 22, 22), 128, 136, 1, ("bf16", 2, 3, 128), ldi=8),
    wg("nt2_ns2_bf16", "bf16", "conv", (2, 36, 36), 256, 192, 9, ("bf16", 2, 2, 128), ldy=8),
]


def wg_geometry(c):
    """(P, in_rows, taps, (N, H, W, Ho, Wo) or None)."""
    if c["op"] == "linear":
        return c["shape"][0], c["shape"][0], 1, None
    N, H, W = c["shape"]
    Ho, Wo = conv_out(H), conv_out(W)
    return N * Ho * Wo, N * H * W, 9, (N, H, W, Ho, Wo)


def wg_case_instance(c):
    P, in_rows, taps, _ = wg_geometry(c)
    return wg_instance(c["dtype"], P, c["Co"], c["Ci"], taps, c["ks"])


def wg_build(c):
    """Operands (Dy [P][Co], In [in_rows][Ci], storage-rounded, CPU) and the float64 weight gradient / S in the slab
    layout [Co][taps * Ci]."""
    tdt, Co, Ci = TDT[c["dtype"]], c["Co"], c["Ci"]
    P, in_rows, taps, conv = wg_geometry(c)
    g = torch.Generator().manual_seed(sum(map(ord, c["id"])))
    if conv is None:
        dy = torch.randn(P, Co, generator=g).to(tdt)
        x = torch.randn(P, Ci, generator=g).to(tdt)
        ref, S = B.ref_and_scale("wgrad_linear", dy, x)
        return dict(Dy=dy, In=x, ref=ref, S=S, P=P, in_rows=in_rows, taps=1, conv=None)
    N, H, W, Ho, Wo = conv
    x = torch.randn(N, Ci, H, W, generator=g).to(tdt)
    dy = torch.randn(N, Co, Ho, Wo, generator=g).to(tdt)
    ref, S = B.ref_and_scale("wgrad_conv2d", dy, x, wshape=(Co, Ci, 3, 3), stride=2)
    slab = lambda t: t.permute(0, 2, 3, 1).reshape(Co, 9 * Ci)                 # [co][kh][kw][ci]
    return dict(Dy=B.rows(dy), In=B.rows(x), ref=slab(ref), S=slab(S), P=P, in_rows=in_rows, taps=9, conv=conv)
