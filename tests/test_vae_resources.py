"""Build-time guards for the VAE filter's kernels (csrc/p3d_vae.h): no scratch, no register spills
to memory, and the LDS a workgroup asks for stays within the device's 160 KiB (no GPU needed)."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "3d-pose-baseline_amd", "libp3d.so")
KERNELS = ("k_vae_fwd(", "k_vae_step(", "k_vae_reduce_adam(", "k_vae_eps(")
LDS_LIMIT = 160 * 1024


def test_vae_kernels_use_no_scratch_and_spill_no_vgprs():
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
        assert r.get("group_segment_fixed_size", 0) == 0, (name, r)    # (their LDS is dynamic: checked below)


def test_vae_lds_is_within_the_device_limit():
    import _p3d

    def lds(i, enc, lat, dec, out):
        e, d = (ctypes.c_int32 * len(enc))(*enc), (ctypes.c_int32 * len(dec))(*dec)
        return _p3d.lib().p3d_vae_lds_bytes(i, len(enc), e, lat, len(dec), d, out)

    default = lds(48, [40, 32], 24, [32, 40], 48)
    assert 0 < default <= LDS_LIMIT
    # at least the packed parameters (8.9 K floats) and four tiles' activations of every layer
    assert default >= 4 * (8904 + 4 * 16 * (40 + 32 + 48 + 24 + 32 + 40 + 48))
    for shape in ((144, [40, 32], 24, [32, 40], 48), (80, [40, 32], 24, [32, 40], 48), (48, [8], 8, [24], 48),
                  (48, [40, 32], 24, [32, 40], 40)):
        assert 0 < lds(*shape) <= LDS_LIMIT, shape
    assert lds(256, [256] * 4, 64, [256] * 4, 64) > LDS_LIMIT     # (refused by p3d_vae_create)
    assert lds(50, [40], 24, [32], 48) == 0
