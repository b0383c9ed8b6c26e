"""Build-time guards for the clip kernels: the single-clip ones (csrc/p3d_clip.h, whose helpers
gained a bounded form), the segmented ones and the batch's index kernel (csrc/p3d_clips.h): no
scratch, no register spills to memory, no dynamic stack, and the static LDS their arrays add up to
(no GPU needed)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "3d-pose-baseline_amd", "libp3d.so")

C, H, NC, T, D = 128, 3, 36, 256, 96            # chunk, halo, columns, threads, the 3D row
MAP = 3 * 64 * 4 + 2 * 64 * 8                   # ClipMap: kind, ca, cb int [64]; mean, stdv double [64]
VOTE = 256                                      # __syncthreads_or's workgroup reduction (clip_lookback)
LDS = {
    # s double [(C + 2H) * NC] | ClipMap | shas int [NC]
    "k_clip_in": (C + 2 * H) * NC * 8 + MAP + NC * 4,
    # s double [C * NC] | smask u64 [T] | sfirst, sfound int [NC] | ClipMap | the vote
    "k_clip_in_carry": C * NC * 8 + T * 8 + 2 * NC * 4 + MAP + VOTE,
    # smean, sstd double [D] | pos int [D] | sox, soz, smx, smn double [C] | sgood, ssrc int [C]
    # (the network's rows [C, U3] float are dynamic)
    "k_clip_out": 2 * D * 8 + D * 4 + 4 * C * 8 + 2 * C * 4,
    # smask u64 [T] | sneed, sfound int [1] | the vote
    "k_clip_out_carry": T * 8 + 2 * 4 + VOTE,
}
KERNELS = [(k.replace("k_clip_", pre) + "(", lds) for k, lds in LDS.items() for pre in ("k_clip_", "k_clips_")]
KERNELS.append(("k_clips_index(", T * 4))       # part int [T]


def test_clip_kernels_use_no_scratch_and_the_lds_they_declare():
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
