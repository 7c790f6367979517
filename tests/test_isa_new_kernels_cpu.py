"""CPU: the listings the build leaves next to its objects (build.py, _check_asm_reads) contain the 64-row gather GEMM
instance with the deep ring and the 12-wave forms of wgrad_gemm_k under the prefixes of build.ISA_CHECKED, and
isa_check.tr_asm_hazards finds nothing in them.  Skipped on a checkout that has not been built."""
import importlib.util
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "symbols-from-video_amd")


def load(name):
    spec = importlib.util.spec_from_file_location("rbvae_" + name, os.path.join(PKG, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def checked_kernels(src):
    """(listing text, prefix, read opcodes, kernel names under the prefix) of a source of build.ISA_CHECKED."""
    path = os.path.join(PKG, "build", src[:-4] + ".s")
    if not os.path.exists(path):
        pytest.skip(path + " is absent: build first")
    prefix, ops = load("build").ISA_CHECKED[src]
    assert isinstance(prefix, str)
    text = open(path).read()
    return text, prefix, ops, set(re.findall(r"^(" + re.escape(prefix) + r"\w+):", text, re.M))


def test_deep_ring_gather_instance_is_checked_and_clean():
    text, prefix, ops, names = checked_kernels("gather_gemm.hip")
    # gather_gemm_k<bf16 (t), 2, 4, RING, 1, 64>, the one type dispatch_gg launches it for (an f32 (f) instance is no longer
    # emitted): the ring is deeper than the three stages it had
    deep = [n for n in names if re.search(r"gather_gemm_kI[tf]Li2ELi4ELi(\d+)ELi1ELi64E", n)]
    assert len(deep) == 1 and "gather_gemm_kIt" in deep[0], sorted(names)
    assert all(int(re.search(r"Li4ELi(\d+)ELi1ELi64E", n).group(1)) > 3 for n in deep), deep
    bad = load("isa_check").tr_asm_hazards(text, prefix, ops)
    assert bad == [], bad[:5]


def test_wgrad_gemm_role_kernels_are_checked_and_clean():
    text, prefix, ops, names = checked_kernels("wgrad_gemm.hip")
    # wgrad_gemm_k<bf16, NT, ring, 128, true>: both widths with the ring of three
    for nt in (1, 2):
        assert any(re.search(r"wgrad_gemm_kItLi%dELi3ELi128ELb1E" % nt, n) for n in names), (nt, sorted(names))
    # and the 8-wave forms the selector keeps reachable
    assert any(re.search(r"wgrad_gemm_kItLi2ELi3ELi128ELb0E", n) for n in names)
    bad = load("isa_check").tr_asm_hazards(text, prefix, ops)
    assert bad == [], bad[:5]
