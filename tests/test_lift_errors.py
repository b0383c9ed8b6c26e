"""Which fault answers, and in what words: the clip, clips and live calls and the two sequence-filter
calls share one host stage (csrc/p3d_clip_host.h, vae_seq_args in csrc/p3d_vae_host.h), and every
refusal they gave before they shared it stays.  tests/golden/lift_errors_parent.json holds (return
code, p3d_last_error) of every bad call of tests/lift_error_cases.py from the library as it stood
with the stage written out per path (tools/record_lift_errors.py); the built library must give the
same pairs.  No GPU: every call is refused before anything is launched."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
LIB = os.path.join(ROOT, "3d-pose-baseline_amd", "libp3d.so")
GOLD = os.path.join(HERE, "golden", "lift_errors_parent.json")

import lift_error_cases  # noqa: E402


@pytest.fixture(scope="module")
def pairs():
    if not os.path.exists(LIB):
        pytest.skip("libp3d.so not built")
    import _p3d
    with open(GOLD) as f:
        want = json.load(f)
    return want, lift_error_cases.run(_p3d.lib()), _p3d.P3D_ERR_ARG


def test_every_refusal_of_the_parent_reproduces(pairs):
    want, got, _ = pairs
    assert [r["id"] for r in got] == [r["id"] for r in want], "the table and the fixture list different calls"
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, "%d of %d calls answer differently, first: want %r, got %r" % (len(bad), len(want), *bad[0])


def test_the_table_is_what_it_says(pairs):
    want, _, E = pairs
    by = {r["id"]: r["msg"] for r in want}
    assert len(want) >= 200 and all(r["rc"] == E for r in want)
    for r in want:                                       # every message names the call that was made
        assert r["msg"].startswith("p3d_" + r["id"].split("/")[0] + ": "), r
    fns = {r["id"].split("/")[0] for r in want}
    assert fns == {"clip_prepare", "clip_finish", "clip_lift", "clips_prepare", "clips_finish", "clips_lift",
                   "live_prepare", "live_finish", "live_push", "vae_seq_filter", "vae_seq_filter_mc",
                   "clips_lift_resampled", "skel_lengths", "skel_pose", "clips_resample"}
    # the two-fault rows the shared stage could most easily turn round
    assert by["clips_lift/null_model_null_statistics"].endswith("null model")            # model first ...
    assert by["live_push/null_statistics"].endswith("null statistics")        # ... and model last
    assert by["live_push/null_model_N0"].endswith("null model")
    assert by["live_push/bad_D3_small_work"].endswith("D3 must be 96 (32 joints)")
    assert by["clip_finish/bad_D3_small_work"].endswith("workspace too small")
    assert "K must be" in by["live_push/bad_K_null_row_off"]
    assert "256-byte aligned" in by["live_push/misaligned_work_filter_arguments"]
    assert by["live_push/global_step_K0"].endswith("null model") and "need a filter" in by["live_push/global_step_K1"]
    assert by["vae_seq_filter/null_filter_global_step"].endswith("null argument")
    assert "ctr may not be P3D_CTR_GLOBAL_STEP" in by["vae_seq_filter_mc/null_filter_global_step"]
    # a row behind a null handle says so in its name and answers with the handle
    for i, msg in by.items():
        if "/null_model" in i and not i.startswith("live_"):
            assert msg.endswith("null model"), (i, msg)
        if i.startswith("vae_seq_filter/null_filter"):
            assert msg.endswith("null argument"), (i, msg)
    assert "need a filter" in by["live_push/ref_var_without_filter"]
    assert "min 9 frames" in by["clip_prepare/smooth_2_frames_null_work"]
    assert "min 9 frames" in by["clips_prepare/smooth_clip_of_8_null_work"]
    # the calls over clip offsets that take no handle: one check of the offsets behind all three
    for fn in ("skel_lengths", "skel_pose", "clips_resample"):
        assert by[fn + "/null_argument_bad_N"].endswith("null argument")
        assert by[fn + "/null_offsets_bad_S"].endswith("null clip offsets")
        assert by[fn + "/bad_S_bad_offsets"].endswith("S must be in 1..N clips")
        assert by[fn + "/empty_then_decreasing"].endswith("clip 0 is empty")
        assert "must not decrease (clip 1)" in by[fn + "/decreasing_then_empty"]
        assert by[fn + "/past_the_end_then_decreasing"].endswith("clip offsets must end at N")
    assert by["skel_lengths/misaligned_work_small"].endswith("null or misaligned workspace")
    assert by["skel_pose/no_outputs_null_offsets"].endswith("null outputs: ask for at least one")
    assert by["clips_resample/R0_clip_of_3"].endswith("R must be in 1..16")
    assert "min 4 frames" in by["clips_resample/clip_of_3_bad_U2"]
    assert by["clips_resample/bad_U2_alias"].endswith("U2 must be in 1..64")
    assert by["clips_resample/alias_null_work"].endswith("xy_r must not alias xy_s")
    assert by["clips_resample/R17_too_many_rows"].endswith("R must be in 1..16")
    assert "R * N must be at most" in by["clips_resample/too_many_rows_long_clip"]
