"""Spline-resampled clips through the lifter (include/p3d.h: p3d_clips_lift_resampled;
ClipLifter.lift_clips(resample=R); the sandbox driver's --spline_resample).

lift_clips(resample = R) is prepare, resample, and p3d_clips_lift on the resampled rows with smooth = 0:
the forward's tiles start again at every clip's first resampled row, so this is an identity of bytes,
checked here against exactly that chain of the existing calls."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-pose-baseline_amd"))
sys.path.insert(0, HERE)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import spline_oracle as so  # noqa: E402
import test_gpu_clip as tc  # noqa: E402  (model_setup, clip_for_model, GOLD, assert_same_bits)
import test_gpu_clips as tcs  # noqa: E402  (lifter_for)
import test_gpu_spline as ts  # noqa: E402  (run: p3d_clips_resample alone)
from top_vae_3d_pose import models  # noqa: E402

LENS, R = [9, 23], 2


@pytest.fixture(scope="module")
def setup():
    st, m, s = tc.model_setup(8)
    vae = models.VAE(144, 24, [40, 32], [32, 40], 48, max_batch=64, seed=17)
    clips = [tc.clip_for_model(n, 500 + n) for n in LENS]
    yield dict(m=m, s=s, vae=vae, clips=clips)
    vae.close()
    m.close()


@pytest.mark.parametrize("cache", [True, False])
@pytest.mark.parametrize("filt", ["none", "filter", "samples"])
def test_lift_clips_resampled_equals_the_chain(setup, filt, cache):
    m, vae, clips = setup["m"], setup["vae"], setup["clips"]
    cl = tcs.lifter_for(m, setup["s"], R * sum(LENS), cache)
    kw = {} if filt == "none" else dict(vae=vae, ctr=77, unfiltered=True, samples=3 if filt == "samples" else None)
    got = cl.lift_clips(clips, resample=R, **kw)
    xy_s = cl.dxy[:sum(LENS)].cpu().numpy()                                  # the smoothed rows the splines were fitted to
    skel = cl.skeleton()
    # prepare then resample, on their own
    plain = cl.lift_clips(clips)
    tc.assert_same_bits(xy_s, np.concatenate([r["xy_s"] for r in plain]), "the smoothed rows")
    alone = ts.run(xy_s, ts.offsets(LENS), R)
    # ... then lift_clips on the resampled clips, unsmoothed
    want = cl.lift_clips([g["xy_s"] for g in got], smooth=False, **kw)
    keys = ["poses", "src", "xy_s"] + ([] if filt == "none" else ["poses_unfiltered", "src_unfiltered"]) + \
        (["ref_var"] if filt == "samples" else [])
    a = 0
    for k, (g, w, n) in enumerate(zip(got, want, LENS)):
        assert sorted(g) == sorted(keys + ["spline_info"]) and sorted(w) == sorted(keys)
        for key in keys:
            assert g[key].shape[0] == R * n
            assert ts.same(g[key], w[key]), "%s of clip %d (%s, cache %s)" % (key, k, filt, cache)
        assert ts.same(g["xy_s"], alone["xy_r"][R * a:R * (a + n)]), "xy_r of clip %d" % k
        assert ts.same(g["spline_info"], alone["info"][k]) and g["spline_info"].shape == (36, 5)
        assert skel[k]["quat"].shape == (R * n, 16, 4) and skel[k]["root"].shape == (R * n, 3)
        a += n
    if filt != "none":
        assert not ts.same(got[1]["poses"], got[1]["poses_unfiltered"])      # the filter ran over the resampled rows
    m.check_errors()


def test_lift_clip_resampled_is_the_batch_of_one(setup):
    cl = tcs.lifter_for(setup["m"], setup["s"], 64)
    poses, xy_r, src, info = cl.lift_clip(setup["clips"][1], resample=R)
    one = cl.lift_clips([setup["clips"][1]], resample=R)[0]
    assert poses.shape == (R * 23, 96) and ts.same(poses, one["poses"]) and ts.same(xy_r, one["xy_s"])
    assert ts.same(src, one["src"]) and ts.same(info, one["spline_info"])
    assert len(cl.skeleton()) == 1 and cl.skeleton()[0]["euler"].shape == (R * 23, 16, 3)
    for bad in (0, 17, 2.5):
        with pytest.raises(ValueError, match="resample"):
            cl.lift_clips(setup["clips"], resample=bad)
    with pytest.raises(ValueError, match="min 4 frames"):
        cl.lift_clips([np.ones((3, 36))], smooth=False, resample=R)


def test_sandbox_driver_spline_resample(tmp_path):
    """--spline_resample 2 on the 23-frame golden clip: 46 frames numbered 0 .. 45, the 2D export the
    oracle's resampling of the reference's own smoothed rows, bit for bit; --interpolation still exits."""
    import openpose_3dpose_sandbox as sandbox
    with np.load(tc.GOLD, allow_pickle=False) as z:
        raw, sm = z["raw_body25_23"], z["sm_body25_23"]
    frames = tmp_path / "json"
    frames.mkdir()
    for i, row in enumerate(raw):
        with open(frames / ("clip_%012d_keypoints.json" % i), "w") as f:
            json.dump({"people": [{"pose_keypoints_2d": [float(v) for v in row]}]}, f)
    base = ["--synthetic", "--residual", "--batch_norm", "--max_batch", "128", "--verbose", "0",
            "--pose_estimation_json", str(frames), "--out_dir", str(tmp_path / "maya")]
    p3, p2 = sandbox.main(base + ["--spline_resample", "2"])[:2]
    three, two = json.load(open(p3)), json.load(open(p2))
    assert sorted(three, key=int) == sorted(two, key=int) == [str(i) for i in range(46)]
    got = np.array([[two[str(i)][str(j)]["translate"] for j in range(18)] for i in range(46)]).reshape(46, 36)
    want = np.stack([so.resample(sm[:, col], 2)["xr"] for col in range(36)], axis=1)
    tc.assert_same_bits(got, want, "the 2D export")
    poses = np.array([[three[str(i)][str(j)]["translate"] for j in range(32)] for i in range(46)])
    assert poses.shape == (46, 32, 3) and np.isfinite(poses).all()
    with pytest.raises(SystemExit, match="spline_resample"):
        sandbox.main(base + ["--interpolation"])
