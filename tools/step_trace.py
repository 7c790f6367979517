"""Every library call of a set of engine passes as text: the engine's counterpart of tools/isa_diff.py.  Two trees whose
engine.py issue the same launches, in the same order, on the same streams, with the same arguments write the same files.

One line per `_lib.call`: entry point, stream (ordinal by first appearance), whether a capture is open, every argument in
position -- scalars verbatim, a tensor as dtype / elements / ordinal of its data_ptr() by first appearance (the tracer keeps
every tensor it has seen, so no address comes back for another one), a gather_gemm class descriptor as its ints, the host
rows of rbvae_run_jobs_table as the table's ordinal, None as None.  Every job table is written at upload, its pointer
columns through the same ordinals.

usage: python tools/step_trace.py --out DIR [--root TREE] [--only SUBSTRING]     one file per case, then count + SHA-256
       python tools/step_trace.py --compare DIR_A DIR_B                          the table of profiles/engine_trace_equal.txt
--root: the tree whose package is traced (default: this one); both trees can load one library through RBVAE_LIB."""
import argparse, ctypes, hashlib, os, sys

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--only", default="")
ap.add_argument("--compare", nargs=2)
a = ap.parse_args()


def digest(path):
    data = open(path, "rb").read()
    return data.count(b"\n"), hashlib.sha256(data).hexdigest()


if a.compare:
    da, db = a.compare
    names = sorted(set(os.listdir(da)) | set(os.listdir(db)))
    bad = 0
    print(f"{'case':36s} {'lines':>6s}  {'sha-256 ' + os.path.basename(da):64s}  {'sha-256 ' + os.path.basename(db):64s}")
    for n in names:
        (ca, ha), (cb, hb) = (digest(os.path.join(d, n)) if os.path.exists(os.path.join(d, n)) else (0, "missing") for d in (da, db))
        bad += ha != hb
        print(f"{n[:-4]:36s} {ca:6d}  {ha:64s}  {hb:64s}  {'equal' if ha == hb else 'DIFFER (%d lines)' % cb}")
    print(f"{len(names)} cases, {bad} differ")
    sys.exit(1 if bad else 0)

root = os.path.abspath(a.root)
sys.path[:0] = [root, os.path.join(root, "tests")]
import torch
import sfv_amd as sfv
from importlib import import_module
import _arms_cases as A
import _lstm_cases as LC
E, J = import_module("symbols-from-video_amd.engine"), import_module("symbols-from-video_amd.jobs")
Col = J.Col
PTR_COLS = {J.JOB_CONV_PACK: (Col.DST2, Col.INNER), J.JOB_ADAM_PACK: (Col.DST2, Col.INNER), J.JOB_ADAM: (Col.INNER,),
            J.JOB_GATHER: (Col.S0, Col.S1)}
DESC_ARG = {"rbvae_gather_gemm": (23, 24)}          # positions of (classes, descriptor address)


class Tracer:
    def __init__(self):
        self.lines, self.ptrs, self.streams, self.tables, self.keep = [], {}, {}, {}, []

    def ptr(self, p):
        return "p%d" % self.ptrs.setdefault(p, len(self.ptrs)) if p else "0"

    def arg(self, x):
        if isinstance(x, torch.Tensor):
            self.keep.append(x)
            return "%s[%d]@%s" % (str(x.dtype)[6:], x.numel(), self.ptr(x.data_ptr()))
        return repr(x)

    def desc(self, ncls, addr):
        out, at = [], 0
        for _ in range(ncls):
            n = ctypes.c_int.from_address(addr + 4 * at).value
            out += [ctypes.c_int.from_address(addr + 4 * (at + i)).value for i in range(3 + 3 * n)]
            at += 3 + 3 * n
        return "desc" + repr(out)

    def call(self, real):
        def traced(name, *args):
            st = self.streams.setdefault(torch.cuda.current_stream().cuda_stream, len(self.streams))
            txt = [self.arg(x) for x in args]
            if name in DESC_ARG:
                n, d = DESC_ARG[name]
                txt[d] = self.desc(args[n], args[d])
            if name == "rbvae_run_jobs_table":
                txt[0] = "table%d" % self.tables[args[0]]
            self.lines.append("%s s%d cap%d %s" % (name, st, torch.cuda.is_current_stream_capturing(), " ".join(txt)))
            return real(name, *args)
        return traced

    def table(self, real):
        tracer = self

        class Traced(real):
            def __init__(self, jl, device, cap):
                super().__init__(jl, device, cap)
                k = tracer.tables.setdefault(self.host_rows.ctypes.data, len(tracer.tables))
                tracer.keep.append(self)
                tracer.lines.append("upload table%d rows %d cap %d" % (k, self.n, cap))
                for r in jl.rows:
                    cols = (Col.SRC, Col.DST) + PTR_COLS.get(r[Col.KIND], ())
                    tracer.lines.append("  " + " ".join(tracer.ptr(v) if i in cols else str(v) for i, v in enumerate(r)))
        return Traced


def traced(fn):
    """The trace of fn(): _lib.call (engine, trainer, jobs and losses reach it as L.call) and the engine's JobTable."""
    t, real_call, real_table = Tracer(), sfv._lib.call, E.JobTable
    sfv._lib.call, E.JobTable = t.call(real_call), t.table(real_table)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        sfv._lib.call, E.JobTable = real_call, real_table
    return t.lines


def model(variant, cin, hw, dtype, latent=32, train=True, seed=5):
    torch.manual_seed(seed)
    return sfv.Seq2SeqBinaryVAE(cin, cin, latent, latent, variant=variant, input_hw=hw, compute_dtype=dtype).cuda().train(train)


def batch(B, T, cin, hw, latent=32, seed=6):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 2, T, cin, *hw, generator=g).cuda(), torch.rand(2, B * T, latent, generator=g).cuda()


def trainer(m, **kw):
    return sfv.FusedTrainer(m, lr=1e-3, alpha=1.0, beta_kl=1.0, bernoulli_p=0.1, noise_ratio=0.1, seed=17, **kw)


def arms(cid, mode):
    def run():
        case = A.BY_ID[cid]
        item, U = A.inputs(case)
        m = model(case["variant"], case["in_ch"], case["hw"], "bf16", train=case["train"], seed=case["model_seed"])
        tr, eng = trainer(m, device_noise=False, use_graph=False), m._engine_for(item.cuda())
        A.lower_thresholds(eng)
        A.switch_off(eng, mode)
        tr.step(item.cuda(), A.TAU, U=U.cuda())
    return run


def steps(dtype, graph, variant="percep", cin=4, hw=(32, 32), B=16, T=8, latent=32, n=2, after=None):
    def run():
        m = model(variant, cin, hw, dtype, latent)
        item, U = batch(B, T, cin, hw, latent)
        tr = trainer(m, device_noise=graph, use_graph=graph)
        for _ in range(n):
            tr.step(item, 0.7, U=None if graph else U)
        if after is not None:
            after(tr, item, U, B, T)
    return run


def autograd(variant, cin, hw, dtype, masks=False):
    def run():
        m = model(variant, cin, hw, dtype)
        item, U = batch(2, 3, cin, hw)
        x = item[:, 0]
        mk = None
        if masks:
            g = torch.Generator().manual_seed(8)
            (c1, c2, _), (H, W) = E.VARIANTS[variant].channels, hw
            sites = [(c1, H // 2, W // 2), (c2, H // 4, W // 4), (c2, H // 4, W // 4), (c1, H // 2, W // 2)]
            mk = [(torch.rand(6, c, h, w, generator=g) > 0.2).float() for c, h, w in sites]
        out = m(x, temperature=0.7, u=U[0], dropout_masks=mk)
        sum(o.float().square().mean() for o in out).backward()
    return run


def inference(tr, item, U, B, T):
    m = tr.model
    m.encode(item[:, 0], temperature=0.5, hard=True, u=U[0])
    m.eval()
    with torch.no_grad():
        m(item[:, 0], temperature=0.5, hard=True, u=U[0])
    tr.validate(item, 0.5, U=U)


def cut(tr, item, U, B, T):
    tr._fwd_bwd(item.contiguous(), U.reshape(2 * B * T, -1).contiguous(), 0.7, B, T, cut=lambda: None)


CASES = {f"arms_{cid}_{mode}": arms(cid, mode) for cid in A.IDS for mode in A.MODES}
for dt in ("bf16", "f32"):
    CASES[f"step_eager_{dt}"] = steps(dt, False)
    CASES[f"step_graph_{dt}"] = steps(dt, True)
    CASES[f"simple_autograd_{dt}"] = autograd("simple", 3, (64, 64), dt)
    CASES[f"contrastive_steps_{dt}"] = steps(dt, False, "contrastive", 3, (48, 80), B=2, T=3)
CASES["percep_masks_autograd_f32"] = autograd("percep", 4, (32, 32), "f32", masks=True)
for what, T in (("pair_bwd_refuses", LC.T_PAIR_BWD_32x4), ("bwd_wave_refuses", LC.T_BWD_32x4), ("fwd_wave_refuses", LC.T_FWD_32x4)):
    CASES[f"long_T{T}_{what}"] = steps("bf16", False, hw=(16, 32), B=1, T=T, n=1)
CASES["latent_50"] = steps("bf16", False, B=4, T=5, latent=50, n=1)
CASES["encode_eval_validate"] = steps("bf16", False, B=4, T=4, n=1, after=inference)
CASES["backward_cut"] = steps("bf16", False, B=4, T=4, n=1, after=cut)

os.makedirs(a.out, exist_ok=True)
for name, fn in CASES.items():
    if a.only in name:
        path = os.path.join(a.out, name + ".txt")
        with open(path, "w") as f:
            f.write("\n".join(traced(fn)) + "\n")
        print("%-36s %6d lines  %s" % ((name,) + digest(path)), flush=True)
