"""Build-time guards for the noise kernel (csrc/p3d_vae_noise.h): no scratch, no register spills to
memory, no dynamic stack, and its static LDS -- the per-wave row lists -- as laid out (no GPU
needed)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "3d-pose-baseline_amd", "libp3d.so")
KERNELS = ("k_vae_noise(",)
# four waves x 64 rows x (source row int64, list entry, joint column, three normals)
STATIC_LDS = 4 * 64 * (8 + 4 + 4 + 3 * 4)


def test_noise_kernel_uses_no_scratch_and_spills_no_vgprs():
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
        assert r.get("group_segment_fixed_size", 0) == STATIC_LDS, (name, r)
        assert r.get("vgpr_count", 0) <= 64, (name, r)       # eight waves per SIMD stay resident
