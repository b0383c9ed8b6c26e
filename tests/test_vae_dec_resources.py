"""Build-time guards for the decoder kernels (csrc/p3d_vae_dec.h): no scratch, no register spills to
memory, no dynamic stack and no static LDS -- their LDS is the dynamic range the host sizes (no GPU
needed)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "3d-pose-baseline_amd", "libp3d.so")
KERNELS = ("k_vae_dec(", "k_vae_bones_dec(")


def test_decoder_kernels_use_no_scratch_and_spill_no_vgprs():
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
        print(name, {k: r.get(k) for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size")})
        assert r.get("private_segment_fixed_size", 0) == 0, (name, r)
        assert r.get("vgpr_spill_count", 0) == 0, (name, r)
        assert not r.get("uses_dynamic_stack", False), (name, r)
        assert r.get("group_segment_fixed_size", 0) == 0, (name, r)
        assert r.get("vgpr_count", 0) <= 128, (name, r)      # four workgroups per CU (one wave each per SIMD) stay resident
