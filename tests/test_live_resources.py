"""Build-time guards for the live kernels (csrc/p3d_live.h): each present exactly once, no scratch,
no register spills to memory, no dynamic stack, and the static LDS their arrays add up to (no GPU
needed)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "3d-pose-baseline_amd", "libp3d.so")

W, NC, D = 4, 36, 96                            # waves (slots) per workgroup, columns, the 3D row
MAP = 3 * 64 * 4 + 2 * 64 * 8                   # ClipMap: kind, ca, cb int [64]; mean, stdv double [64]
KERNELS = [
    # ClipMap | srow double [W, NC]
    ("k_live_in(", MAP + W * NC * 8),
    # smean, sstd double [D] | pos int [D] | sy float [W, D] | sox, soz, smx, smn double [W]
    ("k_live_out(", 2 * D * 8 + D * 4 + W * D * 4 + 4 * W * 8),
]


def test_live_kernels_use_no_scratch_and_the_lds_they_declare():
    if not os.path.exists(LIB):
        pytest.skip("libp3d.so not built")
    if not all(os.path.exists(os.path.join("/opt/rocm/lib/llvm/bin", t))
               for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not present")
    from tools.kernel_resources import kernel_resources
    res = kernel_resources(LIB)
    for name, lds in KERNELS:
        hits = [k for k in res if k.startswith(name)]
        assert len(hits) == 1, "%s: %d kernels in the code object" % (name, len(hits))
        r = res[hits[0]]
        assert r.get("private_segment_fixed_size", 0) == 0, (name, r)
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)
        assert not r.get("uses_dynamic_stack", False), (name, r)
        assert r.get("group_segment_fixed_size", 0) == lds, (name, r, lds)
