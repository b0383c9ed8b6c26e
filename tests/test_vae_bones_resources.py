"""Build-time guards for the bones filter's kernels (csrc/p3d_bones.h and the bones kind of
csrc/p3d_vae.h): no scratch, no register spills to memory, no dynamic stack, no static LDS, and the
dynamic LDS of the default shape within the device's 160 KiB (no GPU needed)."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "3d-pose-baseline_amd", "libp3d.so")
KERNELS = ("k_vae_bones_fwd(", "k_vae_bones_fwd_cat(", "k_vae_bones_step(", "k_vae_bones_step_cat(",
           "k_vae_bones_step_dx(", "void k_bones_from_joints<true>(", "void k_bones_from_joints<false>(",
           "k_bones_to_joints(")
LDS_LIMIT = 160 * 1024


def test_bones_kernels_use_no_scratch_and_spill_no_vgprs():
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
        assert r.get("group_segment_fixed_size", 0) == 0, (name, r)


def test_bones_lds_is_within_the_device_limit():
    import _p3d

    def lds(i, enc, lat, dec):
        e, d = (ctypes.c_int32 * len(enc))(*enc), (ctypes.c_int32 * len(dec))(*dec)
        return _p3d.lib().p3d_vae_bones_lds_bytes(i, len(enc), e, lat, len(dec), d)

    default = lds(1376, [40, 32], 24, [32, 40])
    assert 0 < default <= LDS_LIMIT
    # at least the packed core (everything behind layer 0) and four tiles' activations of every layer
    core = 41 * 32 + 2 * 33 * 24 + 25 * 32 + 33 * 40 + 41 * 16 + 17 * 64
    assert default >= 4 * (core + 4 * 16 * (32 + 48 + 32 + 40 + 16 + 64))
    for shape in ((64, [40, 32], 24, [32, 40]), (264, [8], 8, [8]), (112, [40, 32], 24, [32, 40]),
                  (64, [40, 32, 24, 16], 8, [16, 24, 32, 40])):       # (the last: 11 layers, 26 tensors)
        assert 0 < lds(*shape) <= LDS_LIMIT, shape
    assert lds(256, [256] * 4, 64, [256] * 4) > LDS_LIMIT     # (refused by p3d_vae_create_bones)
    assert lds(50, [40], 24, [32]) == 0
    assert lds(64, [40, 32, 24, 16, 8], 8, [16]) == 0
