"""Build-time guards for the sample kernel (csrc/p3d_sample.h): no scratch, no register spills
to memory, no dynamic stack, and its static LDS as laid out (no GPU needed)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "3d-pose-baseline_amd", "libp3d.so")
# the three instances: float64 input, float32 input read 16 bytes per lane, float32 input unaligned
KERNELS = ("k_sample_world<false, false>(", "k_sample_world<true, true>(", "k_sample_world<true, false>(")
# the [16][96] float64 row image, the [16][96] float32 inputs, R and T of 64 cameras, 96 scatter
# positions, the tile's 16 roots and 16 camera indices
STATIC_LDS = 16 * 96 * 8 + 16 * 96 * 4 + 64 * 12 * 8 + 96 * 4 + 16 * 3 * 8 + 16 * 4


def test_sample_kernel_uses_no_scratch_and_spills_no_vgprs():
    if not os.path.exists(LIB):
        pytest.skip("libp3d.so not built")
    if not all(os.path.exists(os.path.join("/opt/rocm/lib/llvm/bin", t))
               for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not present")
    from tools.kernel_resources import kernel_resources
    res = kernel_resources(LIB)
    for name in KERNELS:
        hits = [k for k in res if name in k]
        assert hits, "%s is not in the code object" % name
        r = res[hits[0]]
        assert r.get("private_segment_fixed_size", 0) == 0, (name, r)
        assert r.get("vgpr_spill_count", 0) == 0, (name, r)
        assert not r.get("uses_dynamic_stack", False), (name, r)
        assert r.get("group_segment_fixed_size", 0) == STATIC_LDS, (name, r)
        # 25,408 bytes of LDS let six workgroups (six waves per SIMD) share a CU's 160 KiB; 80
        # registers (512 / 6, in allocation units of 8) keep the registers from lowering that
        assert r.get("vgpr_count", 0) <= 80, (name, r)
        assert r.get("agpr_count", 0) == 0, (name, r)
