"""CPU: the error model of tests/_loss_cases.py is neither vacuous nor too tight.

* an f32 emulation of every operation (torch float32 in the kernel's order of operations) passes every bound on every case
  of the tables, and its worst |err| / bound per quantity is printed;
* each of the named defects, injected into the emulation, fails at least one case;
* the random tables hold no row within 100 x its bound of a threshold and both hinge branches hold their stated share;
* the float64 gradient model equals torch.autograd of the oracle, exact swap ties included (torch.minimum splits);
* an ambiguous row passes with either branch's output and with nothing else;
* the host hash_u32 reproduces literal values, and the tables reach every kernel."""
import pytest
import torch

import _loss_cases as C
import rbvae_oracle as O

D, F = torch.float64, torch.float32


def merge(dst, prefix, res):
    for k, v in (res.items() if isinstance(res, dict) else [("", res)]):
        key = f"{prefix}.{k}" if k else prefix
        dst[key] = max(dst.get(key, 0.0), v)


# ---- one runner per family: the emulation (with an optional defect) through the checks --------------------------------------

def run_pair(d=None, cases=None):
    out = {}
    for c in cases or C.PAIR_CASES:
        x1, x2 = C.pair_data(c)
        a = (c["label"], c["margin"], c["eps"])
        merge(out, "pairdist_fwd", C.check_pairdist_fwd(x1, x2, *a, C.emu_pairdist_fwd(x1, x2, *a, defect=d), what=c["id"]))
        p1, p2 = C.prev_of(c, "dx1", x1.shape), C.prev_of(c, "dx2", x1.shape)
        g1, g2 = C.emu_pairdist_bwd(x1, x2, *a, c["scale"], c["gs"], p1, p2, defect=d)
        merge(out, "pairdist_bwd", C.check_pairdist_bwd(x1, x2, *a, c["scale"], c["gs"], g1, g2, p1, p2, what=c["id"]))
    return out


def run_cos(d=None):
    out = {}
    for c in C.COS_CASES:
        x1, x2 = C.cos_data(c)
        a = (c["label"], c["margin"], c["eps"])
        merge(out, "paircos_fwd", C.check_paircos_fwd(x1, x2, *a, C.emu_paircos_fwd(x1, x2, *a), what=c["id"]))
        g1, g2 = C.emu_paircos_bwd(x1, x2, *a, c["scale"], c["gs"], defect=d)
        assert torch.isfinite(g1).all() and torch.isfinite(g2).all()
        merge(out, "paircos_bwd", C.check_paircos_bwd(x1, x2, *a, c["scale"], c["gs"], g1, g2, what=c["id"]))
    return out


def run_contrast(d=None):
    out = {}
    for c in C.TERM_CASES:
        h0, h1 = C.term_data(c)
        e = C.emu_contrast(h0, h1, c["scale"], c["gs"], defect=d)
        assert all(torch.isfinite(v).all() for v in e.values())
        merge(out, "contrast_fwd", C.check_contrast_fwd(h0, h1, C.emu_contrast(h0, h1, 1.0, None, defect=d)["out"], what=c["id"]))
        merge(out, "contrast_bwd", C.check_contrast_bwd(h0, h1, c["scale"], c["gs"], e["dh0"], e["dh1"], what=c["id"]))
        merge(out, "contrast_parts", C.check_contrast_parts(h0, h1, e["parts"], what=c["id"]))
    return out


def run_triplet(d=None):
    out = {}
    for c in C.TRIPLET_CASES:
        a, p, n = C.triplet_data(c)
        prev = {k: C.prev_of(c, k, a.shape) for k in "apn"} if c["acc"] else None
        e = C.emu_triplet(a, p, n, c["margin"], c["eps"], c["swap"], c["scale"], c["gs"], prev, defect=d)
        merge(out, "triplet_fwd", C.check_triplet_fwd(a, p, n, c["margin"], c["eps"], c["swap"], e["out"], what=c["id"]))
        merge(out, "triplet_bwd", C.check_triplet_bwd(a, p, n, c["margin"], c["eps"], c["swap"], c["scale"], c["gs"], e, prev, what=c["id"]))
    for c in C.TERM_CASES:
        h0, h1 = C.term_data(c)
        e = C.emu_triplet_term(h0, h1, c["margin"], c["scale"], c["gs"], defect=d)
        assert all(torch.isfinite(v).all() for v in e.values())
        merge(out, "triplet_term_fwd", C.check_triplet_term_fwd(h0, h1, c["margin"], C.emu_triplet_term(h0, h1, c["margin"], 1.0, None)["out"],
                                                              what=c["id"]))
        merge(out, "triplet_term_bwd", C.check_triplet_term_bwd(h0, h1, c["margin"], c["scale"], c["gs"], e["dh0"], e["dh1"], what=c["id"]))
    return out


def kl_parts32(z, p, eps, clamp):
    n = z.numel()
    nb = C.cdiv(n, 256)
    x = torch.zeros(nb * 256)
    x[:n] = C.kl_elem32(z.reshape(-1), p, eps, clamp)
    w = C.wave_sum32(x.view(nb, 4, 64))
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def check_parts(parts, z, p, eps, clamp, what):
    n = z.numel()
    full = n // 256
    r = 0.0
    if full:
        r = C.check_kl_parts(parts[:full], z.reshape(-1)[:full * 256], full, p, eps, clamp, what=what)
    if n % 256:
        r = max(r, C.check_kl_parts(parts[full:], z.reshape(-1)[full * 256:], 1, p, eps, clamp, what=what + " (last block)"))
    return r


def run_binarize(d=None):
    out = {}
    for c in C.BIN_CASES:
        h, Un, gz, prev = C.bin_data(c)
        rows, n = c["rows"], c["rows"] * c["L"]
        if Un is None:
            Un = C.device_uniform(n, c["seed"], c["seed_dev"]).view(h.shape)
        tau = 55.0 if (c["tau_dev"] and d == "tau_dev_ignored") else c["tau"]
        y, z = C.emu_binarize(h, Un, tau, c["ratio"], c["neps"], c["hard"], defect=d)
        assert torch.isfinite(y).all()
        merge(out, "y_soft", C.check_binarize(h, Un, y, z, c["tau"], c["ratio"], c["neps"], c["hard"], what=c["id"]))
        merge(out, "kl_mean", C.check_kl_mean(z, rows, c["p"], c["keps"], c["clamp"],
                                              C.emu_kl_mean(z, rows, c["p"], c["keps"], c["clamp"], defect=d), what=c["id"]))
        merge(out, "kl_parts", check_parts(kl_parts32(z, c["p"], c["keps"], c["clamp"]), z, c["p"], c["keps"], c["clamp"], c["id"]))
        a = (gz, y, z, prev, rows, tau, c["klw"], c["gs"], c["p"], c["keps"], c["clamp"])
        ref_a = a[:5] + (c["tau"],) + a[6:]
        merge(out, "binarize_bwd", C.check_binarize_bwd(*ref_a, C.emu_binarize_bwd(*a, defect=d), what=c["id"]))
    return out


def run_kl(d=None):
    out = {}
    for c in C.KL_CASES:
        v = C.kl_data(c)
        a = (c["rows"], c["p"], c["eps"], c["clamp"])
        merge(out, "kl_fwd", C.check_kl_mean(v, *a, C.emu_kl_mean(v, *a, defect=d), what=c["id"]))
        g = C.emu_kl_bwd(v, *a, c["scale"], c["gs"], defect=d)
        assert torch.isfinite(g).all()
        merge(out, "kl_bwd", C.check_kl_bwd(v, *a, c["scale"], c["gs"], g, what=c["id"]))
    return out


def run_mse(d=None):
    out = {}
    for c in C.MSE_CASES:
        if c["gpu_only"]:
            continue
        a, b = C.mse_data(c)
        merge(out, "mse_fwd", C.check_mse_fwd(a, b, C.emu_mse_fwd(a, b, defect=d), what=c["id"]))
        merge(out, "mse_bwd", C.check_mse_bwd(a, b, c["scale"], c["gs"], C.emu_mse_bwd(a, b, c["scale"], c["gs"]), what=c["id"]))
    return out


def run_combine(d=None):
    out = {}
    for c in C.COMBINE_CASES:
        data = C.combine_data(c)
        merge(out, "combine", C.check_combine(data, C.emu_combine(data, defect=d), what=c["id"]))
        if c["step"] is not None:
            lr = c["lr_dev"] if c["lr_dev"] else c["lr"]
            hy = C.emu_hyper(lr, c["b1"], c["b2"], c["step"] - 1, defect=d)
            merge(out, "hyper", C.check_hyper(hy, lr, c["b1"], c["b2"], c["step"], what=c["id"]))
    return out


def run_adam(d=None):
    out = {}
    for c in C.ADAM_CASES:
        g = C.gen_of(c["n"], c["steps"], 29)
        w, m, v = C.adam_data(c["n"], g, fresh=c["steps"] > 1)
        k = C.adam_consts(c["b1"], c["b2"], c["eps"], c["gscale"])
        for s in range(c["steps"]):
            t = c["t0"] + s + 1
            gr = C.adam_grad(c["n"], g, s)
            if c["mode"] == "step":
                step, bc2 = C.host_hyper(c["lr"], c["b1"], c["b2"], t)
            else:
                hy = C.emu_hyper(c["lr"], c["b1"], c["b2"], t - 1, defect=d)
                merge(out, "hyper", C.check_hyper(hy, c["lr"], c["b1"], c["b2"], t, what=c["id"]))
                step, bc2 = float(hy[0]), float(hy[1])
            w1, m1, v1 = C.emu_adam(w, gr, m, v, k, step, bc2, defect=d)
            assert torch.isfinite(w1).all()
            merge(out, "adam", C.check_adam(C.adam_ref(w, gr, m, v, k, step, bc2), w1, m1, v1, what=f"{c['id']} step {t}"))
            w, m, v = w1, m1, v1
    return out


def run_jobs(d=None, tables=None):
    out = {}
    q = C.JOB_CONSTS
    k = C.adam_consts(q["b1"], q["b2"], q["eps"], q["gscale"])
    step, bc2 = C.host_hyper(q["lr"], q["b1"], q["b2"], q["step"])
    for name in tables or C.JOB_TABLES:
        lay, total, w, gr, m, v = C.table_data(name)
        for j, off in lay:
            sl = slice(off, off + C.job_numel(j))
            w1, m1, v1, copies = C.emu_job(j, w[sl], gr[sl], m[sl], v[sl], k, step, bc2, defect=d)
            merge(out, "job", C.check_job(j, w[sl], gr[sl], m[sl], v[sl], k, step, bc2, w1, m1, v1, copies, what=f"{name}/{j['id']}"))
    return out


FAMILIES = {"pair": run_pair, "cos": run_cos, "contrast": run_contrast, "triplet": run_triplet, "binarize": run_binarize,
            "kl": run_kl, "mse": run_mse, "combine": run_combine, "adam": run_adam, "jobs": run_jobs}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_f32_emulation_passes_every_bound(family):
    res = FAMILIES[family]()
    print(f"\nBOUNDS loss cpu f32 emulation {family}: " + " ".join(f"{k}={v:.3f}" for k, v in res.items()))
    assert res and max(res.values()) <= 1.0
    # a bound the emulation uses to less than 1 % would be slack.  The element-wise bounds are used to 0.2 - 1.0; the scalar
    # sums (fwd, kl_mean, parts, combine) to 0.03 - 0.12: gamma(h) is the worst case of h aligned roundings on every term,
    # the roundings of a sum of thousands of terms are not aligned (a random walk uses ~ 1 / sqrt(terms) of it); a defect
    # in such a sum still lands far outside (test_each_named_defect_fails: 2, 9, 15, 16).  Exempt: the packed copies and
    # hyper terms are exact or a single rounding (ratio 0 is possible), and "job" repeats "adam".
    for k, v in res.items():
        if not k.startswith(("hyper", "job")):
            assert v > 0.01, f"{k}: the emulation reaches only {v:.4f} of the bound"


# (number in the issue's list, defect, family that has to see it)
DEFECTS = [(1, "no_eps", "pair"), (1, "no_eps", "contrast"), (2, "dis_over_BT", "contrast"), (3, "cp_added", "contrast"),
           (4, "last_pair_missing", "contrast"), (5, "swap_to_larger", "triplet"), (6, "hinge_not_zeroed", "triplet"),
           (6, "hinge_not_zeroed", "pair"), (7, "accumulate_ignored", "pair"), (7, "accumulate_ignored", "triplet"),
           (7, "accumulate_ignored", "binarize"), (8, "dx2_plus", "pair"), (9, "kl_mean_over_all", "kl"),
           (9, "kl_mean_over_all", "binarize"), (10, "lp_swapped", "kl"), (11, "clamp_mask_ignored", "kl"),
           (12, "tau_dev_ignored", "binarize"), (13, "no_neps", "binarize"), (14, "cos_no_ia", "cos"), (15, "mse_tail_dropped", "mse"),
           (16, "combine_drops_1024", "combine"), (17, "alpha_beta_exchanged", "combine"), (18, "hyper_for_t", "combine"),
           (18, "hyper_for_t", "adam"), (19, "eps_inside_sqrt", "adam"), (20, "bc2_on_v", "adam"), (21, "gscale_missing_in_v", "adam"),
           (22, "pack_from_old_weight", "jobs"), (23, "ragged_tile_skipped", "jobs"), (0, "tie_to_an", "triplet")]


@pytest.mark.parametrize("num,defect,family", DEFECTS, ids=[f"{n}-{d}-{f}" for n, d, f in DEFECTS])
def test_each_named_defect_fails(num, defect, family):
    """(0, tie_to_an) is triplet_row_bwd as it was before the swap tie was split: the whole gradient to a - n."""
    with pytest.raises(AssertionError):
        FAMILIES[family](defect)


def test_every_listed_defect_is_injected():
    assert {n for n, _, _ in DEFECTS} >= set(range(1, 24))


def test_random_tables_hold_no_ambiguous_row_and_both_branches():
    amb = C.table_ambiguity(K=100.0)
    assert amb and not {k: v for k, v in amb.items() if v}, amb
    shares = C.branch_shares()
    assert len(shares) >= 20
    low = {k: v for k, v in shares.items() if min(v) < C.MIN_SHARE}
    assert not low, low


def test_gradient_model_equals_autograd_of_the_oracle():
    """The float64 references are the oracle's gradients: contrast_term and triplet_term through torch.autograd, on random
    rows and on equal views (exact swap ties, where torch.minimum sends half the gradient each way)."""
    for c in C.TERM_CASES:
        if c["special"] not in (None, "equal-views", "far"):
            continue                                     # d == 0: sqrt has no derivative for autograd
        h0, h1 = C.term_data(c)
        a, b = h0.double().requires_grad_(), h1.double().requires_grad_()
        g0, g1 = torch.autograd.grad(O.contrast_term(a, b) * 0.5, (a, b))
        base, slots, _ = C.contrast_options(h0, h1, 0.5, None)
        ref = base[0].clone()
        for s in slots:                                  # the primary option of every row
            pick = torch.zeros_like(ref)
            done = torch.zeros(ref.shape[0], dtype=torch.bool)
            for r, _, al in s:
                pick = torch.where((al & ~done)[:, None], r, pick)
                done |= al
            ref = ref + pick
        tol = 1e-6 * float(g0.abs().max())
        assert float((ref - g0.reshape(ref.shape)).abs().max()) < tol, c["id"]
        assert float((-base[0] - g1.reshape(ref.shape)).abs().max()) < tol, c["id"]
        a, b = h0.double().requires_grad_(), h1.double().requires_grad_()
        g0, g1 = torch.autograd.grad(O.triplet_term(a, b, c["margin"]) * 2.0, (a, b))
        e = C.emu_triplet_term(h0, h1, c["margin"], 2.0, None)
        scale = max(float(g0.abs().max()), 1e-3)
        assert float((e["dh0"].double() - g0).abs().max()) < 1e-5 * scale, c["id"]
        assert float((e["dh1"].double() - g1).abs().max()) < 1e-5 * scale, c["id"]
        if c["special"] == "equal-views":
            tie = C.emu_triplet_term(h0, h1, c["margin"], 2.0, None, defect="tie_to_an")
            assert float((tie["dh1"].double() - g1).abs().max()) > 1e-2 * scale, "the unsplit tie should differ from autograd"


def test_ambiguous_row_passes_with_either_branch_only():
    """A row whose hinge sits within its bound of the threshold: both branches' outputs pass, a third value does not."""
    L = 16
    x1 = torch.zeros(4, L)
    x2 = torch.zeros(4, L)
    x2[:, 0] = torch.tensor([0.5, 1.0, 1.0, 2.0])
    margin = float(C.Dist(x1, x2, 1e-6).d[1])             # rows 1, 2: m within an f32 rounding of 0, inside the bound
    base, slots, amb = C.pairdist_options(x1, x2, 1, margin, 1e-6, 1.0)
    assert amb.tolist() == [False, True, True, False]
    on, off = slots[0]
    for pick in (on, off):
        got = torch.where(amb[:, None], pick[0], torch.where(on[2][:, None], on[0], off[0]))
        C.check_slots(got.float(), base, slots, 0, "either branch")
    bad = torch.where(on[2][:, None] & ~amb[:, None], on[0], off[0]).clone()
    bad[1, 0] = 1e-3
    with pytest.raises(AssertionError):
        C.check_slots(bad.float(), base, slots, 0, "neither branch")
    got = C.emu_pairdist_bwd(x1, x2, 1, margin, 1e-6, 4.0, None)[0]          # whatever f32 decides, it passes
    C.check_pairdist_bwd(x1, x2, 1, margin, 1e-6, 4.0, None, got, None)


def test_constructed_rows_are_decided_in_f32():
    """a - b + eps == 0 gives d == 0 and a zero gradient; equal views give an exact tie."""
    c = next(c for c in C.PAIR_CASES if c["special"])
    x1, x2 = C.pair_data(c)
    t, d = C.rowdist32(x1, x2, c["eps"])
    assert float(d[0]) == 0.0 and float(C.Dist(x1, x2, c["eps"]).E_d[0]) == 0.0
    g1, _ = C.emu_pairdist_bwd(x1, x2, 1, c["margin"], c["eps"], 1.0, None)
    assert bool((g1[0] == 0).all()) and float(g1[1].abs().max()) / c["eps"] > 1e3       # a == b: the coefficient w m / d ~ 1e6 w / sqrt(L)
    a, p, n = C.triplet_data(next(c for c in C.TRIPLET_CASES if c["special"]))
    T = C.Triplet(a, p, n, 1.0, 1e-8, 1)
    assert bool(T.paths["tie"][0]) and not bool(T.paths["an"][0]) and not bool(T.paths["pn"][0])
    assert float(C.rowdist32(a, n, 1e-8)[1][0]) == float(C.rowdist32(p, n, 1e-8)[1][0])


def test_host_hash_against_literals():
    """hash_u32(seed, idx) of csrc/common.h, worked by hand for (0, 0): x = 1 * GOLD = 0x9E3779B97F4A7C15; x ^= x >> 32 ->
    0x9E3779B9E17D05AC; two rounds of (x *= MIX; x ^= x >> 32) leave the low word 0x001B3979.  The others: the same steps on
    Python integers (hash_u32_by_hand)."""
    x = C.GOLD
    x ^= x >> 32
    assert x == 0x9E3779B9E17D05AC
    lit = {(0, 0): 0x001B3979, (1, 0): 0x8E88561B, (12345, 7): 0x91C067CA, (2 ** 64 - 1, 2 ** 32 + 5): 0xD5E2963E}
    for (seed, idx), want in lit.items():
        assert C.hash_u32_by_hand(seed, idx) == want
        assert int(C.hash_u32(seed, [idx])[0]) == want
    s = ((1 << 63) + 77 + 3 * C.GOLD) & C.M64
    assert int(C.hash_u32(s, [4031])[0]) == 0x3CE67BE8
    u = C.device_uniform(4096, (1 << 63) + 77, 3)
    assert float(u[4031]) == (0x3CE67BE8 >> 8) * 2.0 ** -24 and float(u.min()) >= 0 and float(u.max()) < 1


def test_tables_reach_every_kernel():
    got = C.covered_instances()
    assert got == C.REACHABLE, (sorted(C.REACHABLE - got), sorted(got - C.REACHABLE))
    for L in (1, 16, 25, 32, 50, 63, 64, 65, 100, 128, 200):
        assert any(c["L"] == L for c in C.PAIR_CASES) and any(c["L"] == L for c in C.TERM_CASES)
    assert {c["rows"] for c in C.PAIR_CASES} >= {1, 3, 15, 16, 17, 64, 1000}
    assert {c["T"] for c in C.TERM_CASES} >= {2, 3, 8, 17} and {c["B"] for c in C.TERM_CASES} >= {1, 2, 5, 16}
    assert {c["n"] for c in C.MSE_CASES} == {1, 3, 4, 1027, 2 ** 20 + 3, 2 ** 23 + 1}
    assert {c["n"] for c in C.ADAM_CASES} == {1, 255, 10007, 2048 * 256 + 1}
    for k in ("nparts", "kl_parts", "pair_parts"):
        assert {c[k] for c in C.COMBINE_CASES} == set(C.COUNTS)
    n = [c["rows"] * c["L"] for c in C.BIN_CASES]
    assert min(n) < 8192 < max(n) and 8192 in n and any(x % 256 for x in n)
