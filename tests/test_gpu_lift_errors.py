"""The refusals of p3d_vae_seq_filter / p3d_vae_seq_filter_mc BEHIND a live filter handle: the two
calls share one checked fill of VaeSeqArgs (vae_seq_args, csrc/p3d_vae_host.h), and the order of
its checks and the words of every message are the ones the calls had when each wrote them out.
tests/golden/lift_errors_handle_parent.json holds (return code, p3d_last_error) of
tests/lift_error_cases.handle_cases from that library (tools/record_lift_errors.py --gpu).  Every
call is refused before a launch; its pointers are real device memory all the same."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "lift_errors_handle_parent.json")
GOLD_LIFT = os.path.join(HERE, "golden", "lift_errors_lift_handle_parent.json")

import lift_error_cases  # noqa: E402


def filters():
    from top_vae_3d_pose import models
    return {"seq": models.VAE(144, 24, [40, 32], [32, 40], max_batch=64, seed=3),
            "flat": models.VAE(104, 24, [40, 32], [32, 40], max_batch=64, seed=3),
            "bones": models.VAEBones(64, 8, (24,), (24,), max_batch=64, seed=1)}


def handle_rows():
    """handle_cases against the library _p3d loads, with filters and memory of its own."""
    import torch
    import _p3d
    flt = filters()
    mem = torch.zeros((20 * 16384 + 256,), dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 9, 30], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rows = lift_error_cases.run_handles(_p3d.lib(), {k: m._h for k, m in flt.items()},
                                        (mem.data_ptr() + 255) // 256 * 256, off.data_ptr())
    torch.cuda.synchronize()
    for m in flt.values():
        m.close()
    return rows


def lift_handle_rows():
    """lift_handle_cases against the library _p3d loads: a live model, live filters, and real memory
    behind every pointer (the workspace of the larger call behind the arguments' blocks)."""
    import torch
    import _p3d
    import test_gpu_clip
    lib, block = _p3d.lib(), 32768
    _, model, _ = test_gpu_clip.model_setup(8)
    flt = filters()
    names = lift_error_cases.ORDER["p3d_clips_lift_resampled"].split()
    need = int(lib.p3d_clips_lift_resampled_workspace(30, 2, 2, 32, 48, 1))
    mem = torch.zeros((len(names) * block + need + 256,), dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 9, 30], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rows = lift_error_cases.run_lift_handles(lib, model._h, {k: m._h for k, m in flt.items()},
                                             (mem.data_ptr() + 255) // 256 * 256, off.data_ptr(), block)
    torch.cuda.synchronize()
    for m in list(flt.values()) + [model]:
        m.close()
    return rows


@pytest.mark.gpu
def test_refusals_behind_a_live_filter_are_the_parents():
    import _p3d
    with open(GOLD) as f:
        want = json.load(f)
    got = handle_rows()
    assert len(want) >= 30 and all(r["rc"] == _p3d.P3D_ERR_ARG for r in want)
    assert [r["id"] for r in got] == [r["id"] for r in want]
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, "%d of %d calls answer differently, first: want %r, got %r" % (len(bad), len(want), *bad[0])
    by = {r["id"]: r["msg"] for r in want}
    assert by["vae_seq_filter/bones_bad_S"].endswith("a bones filter has no sequence form")
    assert by["vae_seq_filter_mc/bones_bad_S"].endswith("direction cosines do not average")
    assert by["vae_seq_filter/misaligned_fstate"].endswith("pred, eps, target, state and ref must be 16-byte aligned")
    assert by["vae_seq_filter_mc/misaligned_ref_var"].endswith("state, ref and ref_var must be 16-byte aligned")


@pytest.mark.gpu
def test_refusals_of_the_batched_lifts_behind_live_handles_are_the_parents():
    """p3d_clips_lift and p3d_clips_lift_resampled share one checked argument stage (lift_batch_check,
    csrc/p3d_clip_host.h); tests/golden/lift_errors_lift_handle_parent.json holds what each answered
    when it wrote the checks out itself."""
    import _p3d
    with open(GOLD_LIFT) as f:
        want = json.load(f)
    got = lift_handle_rows()
    assert len(want) >= 60 and all(r["rc"] == _p3d.P3D_ERR_ARG for r in want)
    assert [r["id"] for r in got] == [r["id"] for r in want]
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, "%d of %d calls answer differently, first: want %r, got %r" % (len(bad), len(want), *bad[0])
    by = {r["id"]: r["msg"] for r in want}
    for r in want:
        assert r["msg"].startswith("p3d_" + r["id"].split("/")[0] + ": "), r
    # where the two calls differ, the difference stays
    assert by["clips_lift/bad_D3_alias"].endswith("D3 must be 96 (32 joints)")
    assert by["clips_lift/alias_outputs_without_filter"].endswith("xy_s must not alias xy")
    assert by["clips_lift_resampled/alias_outputs_without_filter"].endswith("xy, xy_s and xy_r must not alias")
    assert by["clips_lift/not_256_small_for_the_call"].endswith("workspace too small")
    assert by["clips_lift_resampled/not_256_small_for_the_call"].endswith("workspace must be 256-byte aligned")
    assert by["clips_lift_resampled/not_256_small_for_the_clips"].endswith("workspace too small")
    for fn in ("clips_lift", "clips_lift_resampled"):
        assert by[fn + "/bones_bad_K"].endswith("a bones filter has no sequence form")
        assert "K must be" in by[fn + "/bad_K_global_step"]
        assert "ctr may not be P3D_CTR_GLOBAL_STEP" in by[fn + "/global_step_K1_src_without_poses"]
        assert by[fn + "/global_step_K0_ref_var"].endswith("ref_var needs K >= 1")
        assert by[fn + "/src_without_poses_bad_row0"].endswith("src_unfiltered needs poses_unfiltered")
        assert by[fn + "/misaligned_eps_null_offsets"].endswith("eps and ref_var must be 16-byte aligned")
        assert "min 9 frames" in by[fn + "/smooth_clip_of_8_null_work"]
    assert by["clips_lift_resampled/smooth_clip_of_8_bad_R"].endswith("min 9 frames for smoothing")
    assert by["clips_lift_resampled/R0_clip_of_3"].endswith("R must be in 1..16")
    assert "min 4 frames" in by["clips_lift_resampled/clip_of_3_not_256"]
