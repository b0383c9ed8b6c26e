"""Build-time guards for k_serve6_rounds (as tests/test_kernel_resources.py for the other hot kernels):
no scratch, no register spills, and its counted post wait follows its refills in the built ISA."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "3d-pose-baseline_amd", "libp3d.so")
NAME = "void k_serve6_rounds<4, 3, 2, 5>"


def _need_tools():
    if not os.path.exists(LIB):
        pytest.skip("libp3d.so not built")
    if not all(os.path.exists(os.path.join("/opt/rocm/lib/llvm/bin", t))
               for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")):
        pytest.skip("ROCm LLVM tools not present")


def test_rounds_kernel_uses_no_scratch_and_matches_the_pair_kernels_lds():
    _need_tools()
    from tools.kernel_resources import kernel_resources
    res = kernel_resources(LIB)
    hits = [k for k in res if k.startswith(NAME)]
    assert hits, "k_serve6_rounds is not in the code object"
    r = res[hits[0]]
    assert r.get("private_segment_fixed_size", 0) == 0, r
    assert r.get("vgpr_spill_count", 0) == 0, r
    assert not r.get("uses_dynamic_stack", False), r
    pair = [k for k in res if k.startswith("void k_serve6<4, 3, 2, 5, true>")]
    assert pair and res[pair[0]]["group_segment_fixed_size"] == r["group_segment_fixed_size"]


def test_rounds_kernel_post_wait_follows_its_refills():
    """The marked `s_waitcnt vmcnt(28)` of the in-contraction post (csrc/p3d_serve6_body.h): walking
    back from every marked wait to the nearest store or label crosses at least 4 (5 + 2) = 28 vector
    loads -- also behind the branches that carry the next round's input layers and the previous
    round's output tiles, whose stores must be acknowledged by that wait like any block's."""
    _need_tools()
    from tools.kernel_resources import kernel_isa
    isa = kernel_isa(NAME, LIB)
    need = 4 * (5 + 2)
    marks = [i for i in range(len(isa) - 1)
             if "s_waitcnt vmcnt(%d)" % need in isa[i] and "s_nop 5" in isa[i + 1]]
    assert marks, "the marked post wait is missing from the rounds kernel"
    vmem = re.compile(r"\s(buffer|global|flat|scratch)_(\w+)")
    label = re.compile(r"^[0-9a-f]{16} <")
    for i in marks:
        loads, j = 0, i - 1
        while j > 0 and not label.match(isa[j]):
            m = vmem.search(isa[j])
            if m and ("store" in m.group(2) or "atomic" in m.group(2)):
                break
            if m:
                loads += 1
            j -= 1
        assert loads >= need, (i, loads, isa[j].strip())
