"""Build-time guards for the K-sample kernels (csrc/p3d_vae_mc.h): they are in the code object, with
no scratch, no register spills to memory, no dynamic stack, and no static LDS beside the dynamic
block (no GPU needed).  All of it is read from the kernels' metadata."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "3d-pose-baseline_amd", "libp3d.so")
KERNELS = ("k_vae_fwd_mc(", "k_vae_fwd_mc_cat(", "k_vae_seq4_mc(")


def test_vae_mc_kernels_use_no_scratch_and_spill_no_vgprs():
    if not os.path.exists(LIB):
        pytest.skip("libp3d.so not built")
    if not all(os.path.exists(os.path.join("/opt/rocm/lib/llvm/bin", t))
               for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not present")
    from tools.kernel_resources import kernel_resources
    res = kernel_resources(LIB)
    for name in KERNELS:
        hits = [k for k in res if k.startswith(name)]
        assert hits, "%s is not in the code object" % name
        r = res[hits[0]]
        assert r.get("private_segment_fixed_size", 0) == 0, (name, r)
        assert r.get("vgpr_spill_count", 0) == 0, (name, r)
        assert not r.get("uses_dynamic_stack", False), (name, r)
        assert r.get("group_segment_fixed_size", 0) == 0, (name, r)    # (their LDS is dynamic)
