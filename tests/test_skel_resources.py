"""Build-time guards for the skeleton kernels (csrc/p3d_skel.h): no scratch, no register spills to
memory, no dynamic stack (no GPU needed)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "3d-pose-baseline_amd", "libp3d.so")

KERNELS = ("k_skel_len_part", "k_skel_len_fold", "k_skel_pose")


def test_skeleton_kernels_use_no_scratch():
    if not os.path.exists(LIB):
        pytest.skip("libp3d.so not built")
    if not all(os.path.exists(os.path.join("/opt/rocm/lib/llvm/bin", t))
               for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not present")
    from tools.kernel_resources import kernel_resources
    res = kernel_resources(LIB)
    for name in KERNELS:
        hits = [k for k in res if k.startswith(name + "(") or k.startswith("void " + name + "<")]
        assert hits, "%s: not in the code object" % name
        for k in hits:                                                    # every instance
            r = res[k]
            assert r.get("private_segment_fixed_size", 0) == 0, (k, r)
            assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, (k, r)
            assert not r.get("uses_dynamic_stack", False), (k, r)
