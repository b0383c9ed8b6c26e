"""Build-time guards for the root trajectory's kernels (csrc/p3d_traj.h): no scratch, no register
spills to memory, no dynamic stack, and the register and LDS figures the gfx950 build reports
(DESIGN.md 8g notes them; no GPU needed)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "3d-pose-baseline_amd", "libp3d.so")

# kernel -> (VGPRs, LDS bytes): k_traj_solve stages 16 rows of 97 + 37 doubles (17,152 bytes; the build
# reports 17,408 with its own padding), k_traj_smooth 320 rows of 3 doubles and a flag
KERNELS = {"k_traj_solve": (44, 17408), "k_traj_smooth": (22, 320 * (3 * 8 + 4))}


def test_trajectory_kernels_use_no_scratch_and_keep_their_figures():
    if not os.path.exists(LIB):
        pytest.skip("libp3d.so not built")
    if not all(os.path.exists(os.path.join("/opt/rocm/lib/llvm/bin", t))
               for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not present")
    from tools.kernel_resources import kernel_resources
    res = kernel_resources(LIB)
    for name, (vgprs, lds) in KERNELS.items():
        hits = [k for k in res if k.startswith(name + "(")]
        assert len(hits) == 1, "%s: one instance in the code object, found %s" % (name, hits)
        r = res[hits[0]]
        assert r.get("private_segment_fixed_size", 0) == 0, (name, r)
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)
        assert not r.get("uses_dynamic_stack", False), (name, r)
        assert r["vgpr_count"] == vgprs and r["agpr_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == lds, (name, r)
