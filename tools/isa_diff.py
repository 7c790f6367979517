#!/usr/bin/env python3
"""Prove that a refactor of csrc/ left the device code alone (CPU only, no GPU needed).

Every csrc/*.hip is compiled to gfx950 assembly twice with build.py's flags: from the working tree, and from a git
revision (--base, default HEAD~1) extracted together with its headers into a temporary directory.  Each listing is
split per kernel symbol (function body plus its .amdhsa_kernel block) and the texts are compared for equality, nothing
else.  Two things are left out of the comparison because they name the source text or the kernel's position in its
file, not its code: lines with the __hip_cuid_<hash> symbol, and the function ordinal <n> inside local labels
(.LBB<n>_<m>, BB<n>_<m> in the loop comments, .Lfunc_end<n>) together with the blanks that pad a label's comment to
its column, so that removing a kernel does not show up as a change of the kernels behind it.

Exit status 0: no kernel changed or was added, and every removed kernel starts with a --removed prefix (mangled or
demangled name).  Anything else: 1, with the kernels listed.

    python tools/isa_diff.py --base HEAD~1 --removed 'rbvae::lstm_wgrad_k' --removed 'rbvae::lstm_fwd_k<64>'
"""
import argparse
import concurrent.futures
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "symbols-from-video_amd"
JOBS = 16

_spec = importlib.util.spec_from_file_location("rbvae_build", os.path.join(ROOT, PKG, "build.py"))
_build = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_build)

_ORDINAL = re.compile(r"(\.LBB|\bBB|\.Lfunc_end|\.Lfunc_begin)\d+")
_PAD = re.compile(r"[ \t]+;")        # a label's comment is padded to a column: the ordinal's digits move it


def extract_base(rev, dest):
    """csrc/ and include/ of `rev`, laid out as in the tree so the relative #includes resolve."""
    names = subprocess.run(["git", "-C", ROOT, "ls-tree", "-r", "--name-only", rev, PKG + "/csrc", "include"],
                           check=True, capture_output=True, text=True).stdout.split("\n")
    for n in filter(None, names):
        path = os.path.join(dest, n)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(subprocess.run(["git", "-C", ROOT, "show", f"{rev}:{n}"], check=True, capture_output=True).stdout)
    return os.path.join(dest, PKG, "csrc")


def compile_asm(job):
    src, out = job
    cmd = [_build.HIPCC] + _build.FLAGS + ["-S", "--cuda-device-only", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc -S failed on {src}:\n{r.stderr}")
    return out


def kernels(asm):
    """{kernel symbol: function body + .amdhsa_kernel block} of one listing."""
    lines = [_PAD.sub(" ;", _ORDINAL.sub(lambda m: m.group(1), ln)) for ln in asm.split("\n") if "__hip_cuid_" not in ln]
    names = [ln.split()[1] for ln in lines if ln.startswith("\t.amdhsa_kernel ")]
    out = {}
    for name in names:
        body = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(i for i in range(body, len(lines)) if lines[i].startswith(".Lfunc_end"))
        desc = lines.index("\t.amdhsa_kernel " + name)
        dend = next(i for i in range(desc, len(lines)) if lines[i].startswith("\t.end_amdhsa_kernel"))
        out[name] = "\n".join(lines[body:end + 1] + lines[desc:dend + 1])
    return out


def demangle(names):
    if not names:
        return {}
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    plain = r.stdout.split("\n") if r.returncode == 0 else names
    return dict(zip(names, plain))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--base", default="HEAD~1", help="git revision to compare the working tree against")
    ap.add_argument("--removed", action="append", default=[], metavar="PREFIX",
                    help="a kernel whose mangled or demangled name starts with PREFIX may be gone (repeatable)")
    args = ap.parse_args()

    with tempfile.TemporaryDirectory() as tmp:
        base_csrc = extract_base(args.base, os.path.join(tmp, "base"))
        sides = {"base": base_csrc, "tree": os.path.join(ROOT, PKG, "csrc")}
        jobs = []
        for side, d in sides.items():
            os.makedirs(os.path.join(tmp, "asm", side))
            jobs += [(os.path.join(d, f), os.path.join(tmp, "asm", side, f[:-4] + ".s"))
                     for f in sorted(os.listdir(d)) if f.endswith(".hip")]
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(JOBS, os.cpu_count() or 2)) as ex:
            list(ex.map(compile_asm, jobs))
        found = {side: {} for side in sides}
        for side in sides:
            d = os.path.join(tmp, "asm", side)
            for f in sorted(os.listdir(d)):
                for k, text in kernels(open(os.path.join(d, f)).read()).items():
                    found[side][(f[:-2] + ".hip", k)] = text

    base, tree = found["base"], found["tree"]
    changed = sorted(k for k in base.keys() & tree.keys() if base[k] != tree[k])
    added = sorted(tree.keys() - base.keys())
    removed = sorted(base.keys() - tree.keys())
    plain = demangle([k for _, k in changed + added + removed])
    # a template kernel demangles with its return type in front: "void rbvae::lstm_fwd_k<64>(float const*, ...)"
    names = {k: (k[1], plain[k[1]], plain[k[1]].removeprefix("void ")) for k in removed}
    unexpected = [k for k in removed if not any(n.startswith(p) for n in names[k] for p in args.removed)]

    print(f"isa_diff: working tree against {args.base}: {len(base)} kernels before, {len(tree)} after")
    for title, keys in (("changed", changed), ("added", added), ("removed", removed)):
        print(f"{title}: {len(keys) or 'none'}")
        for f, k in keys:
            print(f"  {f}: {plain[k]}" + ("   <-- not on the --removed list" if title == "removed" and (f, k) in unexpected else ""))
    bad = bool(changed or added or unexpected)
    print("FAIL" if bad else "OK")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
