"""The two-product sites behind c_k of the fp64 wavefront control kernel keep the fusion they are pinned to
(csrc/control_wave_impl.hpp mul_add / mul_sub / __builtin_fma; profiles/wave_trim.txt rung 1): the co-state sums
a02 (...) + a12 (...), v0 = cth r0 + sth r1 and the Rinv products of the update.  Which product the compiler fuses where two
meet in one add is its own choice by use counts, code far from the site can move it, and 50 receding-horizon steps of clamped
controls turn the one unit in the last place into sign flips -- so the form is written down and checked here, without a GPU:
the four lean K = 5 / 10 instances are compiled to gfx950 ISA with the flags of control_wave_kernel.o and their fp64
instructions are read as expression trees (tools/wave_fp64_trees.py).  cos / sin of the parked heading are told apart by their
LDS offsets: sin lies kMaxS * 64 doubles = 2048 bytes behind cos.  Nothing else is looked for in the assembly.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ergodic_exploration_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import wave_fp64_trees as trees

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SIN_BEHIND_COS = 4 * 64 * 8  # bytes: s_sp = s_cp + kMaxS * kWave
INSTANCES = [("simple_cart", 1, 10), ("omni", 0, 10), ("simple_cart", 1, 5), ("omni", 0, 5)]


def wave_object_flags():
    """what csrc/Makefile compiles control_wave_kernel.o with, beyond the common flags"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"control_wave_kernel\.o: OBJFLAGS := (.*?) \$\(WAVE_EXTRA\)", mk)
    assert m, "csrc/Makefile: the flags of control_wave_kernel.o"
    return m.group(1).split()


@pytest.fixture(scope="module")
def instance_trees(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("wave_isa")
    src = d / "instances.hip"
    src.write_text('#include "control_wave_impl.hpp"\nnamespace eea { namespace wave {\n' + "".join(
        "template __global__ void control_wave_kernel<double, %d, %d, false, 4, false>(const ControlParams<double>, "
        "const unsigned, const int, const int);\n" % (m, k) for _, m, k in INSTANCES) + "} }\n")
    out = d / "instances.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950"] + wave_object_flags() +
                   ["--cuda-device-only", "-S", "-I", CSRC, str(src), "-o", str(out)], check=True, capture_output=True)
    ks = trees.kernels(str(out))
    res = {}
    for name, m, k in INSTANCES:
        sym = [s for s in ks if "kernelIdLi%dELi%dELb0ELi4ELb0E" % (m, k) in s]
        assert len(sym) == 1, (name, k, sorted(ks))
        res[(name, k)] = trees.trees_of(ks[sym[0]], 3)
    return res


def first_offsets(tree):
    """LDS offsets of the first value read from LDS in the fused product and in the addend of fma(P, A)"""
    depth, cut = 0, None
    for i, c in enumerate(tree):
        depth += c == "("
        depth -= c == ")"
        if c == "," and depth == 1:
            cut = i
            break
    assert cut is not None, tree
    p, a = re.search(r"lds:(\d+)", tree[:cut]), re.search(r"lds:(\d+)", tree[cut:])
    return (int(p.group(1)) if p else None), (int(a.group(1)) if a else None)


@pytest.mark.parametrize("model,m,K", INSTANCES, ids=["%s_K%d" % (n, k) for n, _, k in INSTANCES])
def test_pinned_sites_keep_their_fusion(instance_trees, model, m, K):
    t = instance_trees[(model, K)]
    # v0 = cth r0 + sth r1: cth r0 is fused, sth r1 is rounded
    v0 = [s for s in t if re.match(r"^fma\(lds:\d+\*v_add_f64\(.*\),-?mul\(lds:\d+,v_add_f64\(N,N\)\)\)$", s)]
    # the co-state sums: the a02 product (its heading factor is the sine) is fused, the a12 product is rounded
    if model == "simple_cart":
        co = [s for s in t if re.match(r"^fma\(-(L\*)?mul\(L,lds:\d+\)(\*v_add_f64\(.*\))?,mul\((L,)?mul\(L,lds:\d+\)", s)]
    else:
        co = [s for s in t if re.match(r"^fma\((L\*)?fma\(-L\*lds:\d+,-mul\(L,lds:\d+\)\)(\*v_add_f64\(.*\))?,"
                                       r"mul\((L,)?fma\(L\*lds:\d+,-N\)", s)]
    print(model, K, "v0 sites", len(v0), "co-state sites", len(co))
    assert len(v0) >= 3 and len(co) >= 6, (v0, co)
    for s in v0:
        p, a = first_offsets(s)
        assert a - p == SIN_BEHIND_COS, s
    for s in co:
        p, a = first_offsets(s)
        assert p - a == SIN_BEHIND_COS, s
    # u_r = Rinv[r] n0 + Rinv[r + 3] n1 + Rinv[r + 6] n2: Rinv[r] n0 (n0 = -v0) is rounded, the other two are fused
    rounded = sum(n for s, n in t.items() if re.match(r"^fma\(.*,-mul\(fma\(N\*lds:\d+,N\),s\)\)$", s))
    fused = [s for s in t if re.match(r"^fma\(-?fma\(N\*lds:\d+,N\)\*s,", s)]
    print(model, K, "Rinv sites with the v0 product rounded", rounded, "fused", len(fused))
    assert rounded >= 9 and not fused, (rounded, fused)
