"""The root trajectory on the GPU (include/p3d.h: p3d_root_trajectory; ClipLifter.trajectory,
trajectory_rows, export_trajectory, the drivers' --root_trajectory) against tests/traj_oracle.py,
which states the same float64 operations in numpy.

Tolerances: valid exact; T, its windowed mean and resid 1e-9 max(1, |value|) -- the chains are a few
dozen correctly rounded operations (unit roundoff 1.1e-16), the solve divides by D >= 1e-4 on the
synthetic rows (asserted), so the expected error is around 1e-13.  On the synthetic rows the GPU gave
the oracle's bytes, so there the comparison is tightened to bytes (check_against_oracle); the lifted
rows of the end-to-end test keep the 1e-9 bound.  Everything said to be the same bits is compared as
bytes."""
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

import _p3d  # noqa: E402
import openpose_frontend as of  # noqa: E402
import skel_oracle as so  # noqa: E402  (read_bvh)
import test_gpu_clip as tc  # noqa: E402  (clip_for_model, USE2, IGN3)
import test_gpu_skel as tgs  # noqa: E402  (small_model, write_clip, tree, the drivers' checkpoint)
import traj_oracle as to  # noqa: E402
from test_gpu_skel import driver  # noqa: E402,F401  (the fixture)

W = int(_p3d.lib().p3d_root_trajectory_rows())
OUTS = (("traj", 3, torch.float64), ("traj_raw", 3, torch.float64), ("resid", 1, torch.float64), ("valid", 1, torch.int32))
GUARD, SENTINEL = 64, -7                                 # guard words around every output and the workspace
CAM = (to.F, to.CX, to.CY)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def run(poses, xy, src, off, h, want=("traj", "traj_raw", "resid", "valid"), off_dev=None, cam=CAM):
    """The call on fresh buffers with guard words around every output and the workspace -> dict of the
    outputs asked for."""
    lib, p = _p3d.lib(), _p3d.ptr
    off = np.ascontiguousarray(off, np.int64)
    S, N = len(off) - 1, int(off[-1])
    d_poses = torch.from_numpy(np.ascontiguousarray(poses, np.float64)).cuda()
    d_xy = torch.from_numpy(np.ascontiguousarray(xy, np.float64)).cuda()
    d_src = None if src is None else torch.from_numpy(np.asarray(src, np.int32)).cuda()
    d_off = torch.from_numpy(off if off_dev is None else np.ascontiguousarray(off_dev, np.int64)).cuda()
    bufs = {k: torch.full((N * w + 2 * GUARD,), SENTINEL, dtype=dt, device="cuda") for k, w, dt in OUTS if k in want}
    ptr = lambda t: p(t) + GUARD * t.element_size()   # noqa: E731
    nbytes = int(lib.p3d_root_trajectory_workspace(N, h))
    work = torch.full((nbytes // 8 + 2 * GUARD,), float(SENTINEL), dtype=torch.float64, device="cuda")
    _p3d.check(lib.p3d_root_trajectory(p(d_poses), p(d_xy), p(d_src), off.ctypes.data, p(d_off), S, N, *cam, h,
                                       *(ptr(bufs[k]) if k in want else None for k, _, _ in OUTS),
                                       ptr(work) if nbytes else None, nbytes, _p3d.stream_handle()), "p3d_root_trajectory")
    torch.cuda.synchronize()
    out = {}
    for k, t in list(bufs.items()) + [("work", work)]:
        g = t.cpu().numpy()
        assert (g[:GUARD] == SENTINEL).all() and (g[-GUARD:] == SENTINEL).all(), "%s: a guard word changed" % k
        out[k] = g[GUARD:-GUARD]
    del out["work"]
    shapes = dict(traj=(N, 3), traj_raw=(N, 3), resid=(N,), valid=(N,))
    return {k: v.reshape(shapes[k]) for k, v in out.items()}


def check_against_oracle(got, poses, xy, src, off, h, what=""):
    """valid exact; T, its windowed mean and resid the oracle's BYTES wherever the oracle has no NaN, NaN
    exactly where it has one (a NaN's sign and payload are not part of the definition).  The first GPU
    run showed byte equality on every synthetic row (MEASUREMENTS.md), so the comparison is bytes,
    inside the 1e-9 max(1, |value|) the definition allows."""
    want = to.trajectory(poses, xy, src, off, *CAM, h)
    np.testing.assert_array_equal(got["valid"], want["valid"], what)
    for k in ("traj_raw", "traj", "resid"):
        worst = to.close(got[k], want[k], "%s %s" % (what, k))
        nan = np.isnan(want[k])
        print("%s %s: worst error %.3e" % (what, k, worst))
        assert same(got[k][~nan], want[k][~nan]), "%s %s: not the oracle's bytes (worst error %.3e)" % (what, k, worst)
    return want


@pytest.mark.parametrize("n", [1, 9, W - 1, W, W + 1, 2 * W + 3])
def test_single_clip_matches_the_oracle(n):
    poses, xy, T = to.synth(n, 100 + n)
    assert to.solve(poses, xy, None, *CAM)[3].min() > 1e-4   # no row near the degenerate branch: nothing left out
    off = offsets([n])
    for h in (0, 4):
        got = run(poses, xy, np.arange(n), off, h)
        check_against_oracle(got, poses, xy, None, off, h, "%d frames, h = %d" % (n, h))
        assert got["valid"].all()
        again = run(poses, xy, np.arange(n), off, h)
        for k in got:
            assert same(got[k], again[k]), "%s differs between two identical calls" % k
        null = run(poses, xy, None, off, h)                  # a null src: every row its own
        for k in got:
            assert same(got[k], null[k]), "%s with a null src" % k
    assert same(run(poses, xy, None, off, 0)["traj"], got["traj_raw"])        # h = 0: the raw bytes
    to.close(got["traj_raw"], T, "the translation the rows were made with")


@pytest.mark.parametrize("h", [4, 32])
def test_batch_carries_the_single_clip_bits_and_wrong_offsets_stay_inside(h):
    lens = [1, 2, h, h + 1, 2 * h + 1, W + 1]
    off, N = offsets(lens), sum(lens)
    poses, xy, _ = to.synth(N, 7 + h)
    src = np.arange(N)
    src[off[4] + 3] = -1                                     # an invalid row inside a window
    got = run(poses, xy, src, off, h)
    check_against_oracle(got, poses, xy, src, off, h, "batch, h = %d" % h)
    again = run(poses, xy, src, off, h)
    for k in got:
        assert same(got[k], again[k]), "%s differs between two identical calls" % k
    for s, (a, b) in enumerate(zip(off[:-1], off[1:])):
        local = np.where(src[a:b] >= 0, src[a:b] - a, -1)
        one = run(poses[a:b], xy[a:b], local, offsets([b - a]), h)
        for k in got:
            assert same(one[k], got[k][a:b]), "%s of clip %d (%d frames)" % (k, s, b - a)
    # a wrong device copy of the offsets changes rows only: the guards (checked in run) are unchanged
    S = len(lens)
    for wrong in ([0, 5, 3, N + 900, N, 1, 2], [-40, 1 << 40, -1, 7, 2, 0, 9], [N] * (S + 1), [0] * (S + 1), [0] + [N] * S):
        out = run(poses, xy, src, off, h, off_dev=wrong)
        assert out["traj"].shape == (N, 3) and same(out["traj_raw"], got["traj_raw"])


def test_special_rows_at_a_workgroups_first_and_last_row():
    lens = [3 * W, 2 * W + 5]
    off, N = offsets(lens), sum(lens)
    poses, xy, T = to.synth(N, 21)
    src = np.arange(N)
    held, zero, degen, nan = (W, 2 * W - 1), (2 * W, 3 * W - 1), (3 * W, 4 * W - 1), (4 * W, 5 * W - 1)
    for n in held:                                           # shows the row before it; its own detections failed
        src[n], poses[n], xy[n] = n - 1, poses[n - 1], 0.0
    for n in zero:
        src[n], poses[n] = -1, 0.0
    for n in degen:
        xy[n] = np.tile([400.0, 300.0], 18)
    for n in nan:
        poses[n, 3 * 17 + 2] = np.nan
    for h in (0, 4):
        got = run(poses, xy, src, off, h)
        want = check_against_oracle(got, poses, xy, src, off, h, "special rows, h = %d" % h)
        for n in zero + degen:
            assert got["valid"][n] == 0 and got["resid"][n] == 0.0 and not got["traj_raw"][n].any() and not got["traj"][n].any()
        for n in held:
            assert got["valid"][n] == 1 and same(got["traj_raw"][n], got["traj_raw"][n - 1]) and got["resid"][n] == got["resid"][n - 1]
        for n in nan:
            assert got["valid"][n] == 1 and np.isnan(got["traj_raw"][n]).all() and np.isnan(got["resid"][n])
        assert np.isnan(want["traj_raw"]).any(axis=1).sum() == len(nan)
    # a zero row whose buffers hold something else still counts as zeros
    junk = poses.copy()
    junk[list(zero)] = np.random.default_rng(1).uniform(-500.0, 500.0, (2, 96))
    for k, v in run(junk, xy, src, off, 4).items():
        assert same(v, got[k]), k


def test_each_output_alone_gives_the_same_bits():
    lens = [W + 3, 17]
    off, N = offsets(lens), sum(lens)
    poses, xy, _ = to.synth(N, 33)
    src = np.arange(N)
    src[5], poses[5] = 4, poses[4]
    src[W] = -1
    for h in (0, 4):
        both = run(poses, xy, src, off, h)
        for k, _, _ in OUTS:
            alone = run(poses, xy, src, off, h, want=(k,))
            assert sorted(alone) == [k] and same(alone[k], both[k]), "%s on its own, h = %d" % (k, h)
        pair = run(poses, xy, src, off, h, want=("traj", "resid"))
        assert same(pair["traj"], both["traj"]) and same(pair["resid"], both["resid"])


def test_trajectory_rows_takes_the_lifters_local_src():
    lens = [12, 9]
    off, N = offsets(lens), sum(lens)
    poses, xy, _ = to.synth(N, 44)
    local = np.concatenate([np.arange(n) for n in lens]).astype(np.int32)
    local[13], poses[13] = -1, 0.0                           # clip 1, position 1: zeros
    local[15], poses[15] = 2, poses[14]                      # clip 1, position 3 shows position 2
    glob = np.where(local >= 0, local + np.repeat(off[:-1], lens), -1)
    res = of.trajectory_rows(poses, xy, local, off, to.F, (to.CX, to.CY), smooth_half=4)
    want = run(poses, xy, glob, off, 4)
    for s, r in enumerate(res):
        assert sorted(r) == ["camera", "resid", "root_skel", "traj", "traj_raw", "valid"]
        a, b = off[s], off[s + 1]
        for k in ("traj", "traj_raw", "resid"):
            assert same(r[k], want[k][a:b]), k
        assert r["valid"].dtype == np.bool_ and (r["valid"] == (want["valid"][a:b] != 0)).all()
        t = r["traj"]
        assert (r["root_skel"] == np.stack([t[:, 0], -t[:, 1], -t[:, 2]], axis=1)).all()
        assert r["camera"] == dict(focal=to.F, center=[to.CX, to.CY], smooth_half=4)
    assert not res[1]["valid"][1] and res[1]["valid"][3]
    for bad in (dict(poses=poses[:, :95]), dict(xy_s=xy[:-1]), dict(xy_s=xy[:, :35]), dict(offsets=[0, 5]),
                dict(offsets=[0, 0, N]), dict(src=local[:-1]), dict(src=np.full(N, 12)), dict(focal=0.0),
                dict(center=(1.0, np.nan)), dict(smooth_half=33)):
        kw = dict(dict(poses=poses, xy_s=xy, src=local, offsets=off, focal=to.F, center=(to.CX, to.CY), smooth_half=4), **bad)
        with pytest.raises(ValueError):
            of.trajectory_rows(**kw)


# ---- end to end ---------------------------------------------------------------------------------
def test_lift_clips_then_trajectory():
    m, s = tgs.small_model()
    lens = [23, 12, W + 9]
    clips = [tc.clip_for_model(n, 60 + n) for n in lens]
    cl = of.ClipLifter(m, s["mean2"], s["std2"], tc.USE2, s["mean3"], s["std3"], tc.IGN3, max_frames=sum(lens))
    with pytest.raises(ValueError, match="no lift"):
        cl.trajectory(to.F, (to.CX, to.CY))
    for resample in (None, 2):
        res = cl.lift_clips(clips, resample=resample)
        got = cl.trajectory(to.F, (to.CX, to.CY), smooth_half=4)
        R = resample or 1
        off = offsets([R * n for n in lens])
        poses, xy = np.concatenate([r["poses"] for r in res]), np.concatenate([r["xy_s"] for r in res])
        local = np.concatenate([r["src"] for r in res])
        rows = of.trajectory_rows(poses, xy, local, off, to.F, (to.CX, to.CY), smooth_half=4)
        glob = np.where(local >= 0, local + np.repeat(off[:-1], np.diff(off)), -1)
        want = to.trajectory(poses, xy, glob, off, *CAM, 4)
        for c, (g, r) in enumerate(zip(got, rows)):
            assert len(g["traj"]) == R * lens[c]
            for k in ("traj", "traj_raw", "resid", "valid", "root_skel"):
                assert same(g[k], r[k]), "%s of clip %d, resample %s" % (k, c, resample)
            assert (g["valid"] == (want["valid"][off[c]:off[c + 1]] != 0)).all()
            for k in ("traj", "traj_raw", "resid"):
                to.close(g[k], want[k][off[c]:off[c + 1]], "%s of clip %d against the oracle" % (k, c))
        if resample is None:
            assert (local == -1).any() and ((local >= 0) & (local != np.concatenate([np.arange(n) for n in lens]))).any()
    p1, x1, s1 = cl.lift_clip(clips[0])                      # a single clip
    one = cl.trajectory(to.F, (to.CX, to.CY), smooth_half=4)
    rows = of.trajectory_rows(p1, x1, s1, [0, lens[0]], to.F, (to.CX, to.CY), smooth_half=4)
    assert len(one) == 1 and same(one[0]["traj"], rows[0]["traj"]) and same(one[0]["resid"], rows[0]["resid"])
    m.check_errors()
    m.close()


def bvh_motion(path):
    _, ft, motion = so.read_bvh(path)
    return ft, motion


def trajectory_of_the_export(paths, n):
    """A driver's trajectory.json against trajectory_rows of the 3d_data.json / 2d_data.json beside it at
    the default window (4) -> that result."""
    three, two = json.load(open(paths[0])), json.load(open(paths[1]))
    poses = np.array([[three[str(i)][str(j)]["translate"] for j in range(32)] for i in range(n)]).reshape(n, 96)
    xy = np.array([[two[str(i)][str(j)]["translate"] for j in range(18)] for i in range(n)]).reshape(n, 36)
    assert poses.any(axis=1).all()                           # no zero row: every frame carries its own pose
    want = of.trajectory_rows(poses, xy, None, [0, n], 1145.0, (512.0, 515.0), smooth_half=4)[0]
    tj = json.load(open(paths[3]))
    assert sorted(tj) == ["camera", "resid", "trajectory", "valid"]
    assert tj["camera"] == {"focal": 1145.0, "center": [512.0, 515.0], "smooth_half": 4}
    assert same(np.array([tj["trajectory"][str(i)] for i in range(n)]), want["traj"])
    assert same(np.array(tj["resid"]), want["resid"]) and tj["valid"] == want["valid"].tolist() and all(tj["valid"])
    return want


CAMERA_FLAGS = ["--root_trajectory", "--focal", "1145", "--principal", "512", "515"]


def test_sandbox_driver_root_trajectory(driver, tmp_path):   # noqa: F811
    import openpose_3dpose_sandbox as sandbox
    root, names, base = driver
    one = ["--pose_estimation_json", str(root / "b_twelve")]
    plain = sandbox.main(base + one + ["--out_dir", str(tmp_path / "plain"), "--export_bvh"])
    assert tgs.tree(str(tmp_path / "plain")) == ["2d_data.json", "3d_data.json", "skeleton.bvh"]
    got = sandbox.main(base + one + ["--out_dir", str(tmp_path / "traj"), "--export_bvh"] + CAMERA_FLAGS)
    assert [os.path.basename(q) for q in got] == ["3d_data.json", "2d_data.json", "skeleton.bvh", "trajectory.json"]
    assert tgs.tree(str(tmp_path / "traj")) == ["2d_data.json", "3d_data.json", "skeleton.bvh", "trajectory.json"]
    for a, b in zip(plain[:2], got[:2]):                     # the flag changes nothing else
        assert open(a, "rb").read() == open(b, "rb").read()
    want = trajectory_of_the_export(got, 12)
    # the BVH's root columns are root_skel; every other column and line is the plain BVH's
    (ft0, m0), (ft1, m1) = bvh_motion(plain[2]), bvh_motion(got[2])
    assert ft0 == ft1 and same(m1[:, :3], want["root_skel"]) and same(m1[:, 3:], m0[:, 3:]) and not same(m1[:, :3], m0[:, :3])
    head = lambda path: open(path).read().split("MOTION")[0]   # noqa: E731
    assert head(plain[2]) == head(got[2])
    # without --export_bvh: trajectory.json alone beside the two files, the same bytes; a batch of clips
    only = sandbox.main(base + ["--clips_root", str(root), "--out_dir", str(tmp_path / "clips"), "--trajectory_smooth", "4"]
                        + CAMERA_FLAGS)
    assert tgs.tree(str(tmp_path / "clips")) == sorted(os.path.join(c, f) for c in names
                                                       for f in ("2d_data.json", "3d_data.json", "trajectory.json"))
    assert open(only[1][2], "rb").read() == open(got[3], "rb").read()
    assert open(only[1][0], "rb").read() == open(got[0], "rb").read()


def test_realtime_driver_root_trajectory(driver, tmp_path):   # noqa: F811
    import openpose_3dpose_sandbox_realtime as rt
    root, names, base = driver
    live = base + ["--pose_estimation_json", str(root / "b_twelve"), "--idle_exit", "0", "--export_bvh"]
    plain = rt.main(live + ["--out_dir", str(tmp_path / "plain")])
    assert tgs.tree(str(tmp_path / "plain")) == ["2d_data.json", "3d_data.json", "skeleton.bvh"]
    got = rt.main(live + ["--out_dir", str(tmp_path / "live")] + CAMERA_FLAGS)
    assert [os.path.basename(q) for q in got] == ["3d_data.json", "2d_data.json", "skeleton.bvh", "trajectory.json"]
    assert tgs.tree(str(tmp_path / "live")) == ["2d_data.json", "3d_data.json", "skeleton.bvh", "trajectory.json"]
    for a, b in zip(plain[:2], got[:2]):                     # the flag changes nothing else
        assert open(a, "rb").read() == open(b, "rb").read()
    want = trajectory_of_the_export(got, 12)                 # at export time, from the collected rows
    (ft0, m0), (ft1, m1) = bvh_motion(plain[2]), bvh_motion(got[2])
    assert ft0 == ft1 and same(m1[:, :3], want["root_skel"]) and same(m1[:, 3:], m0[:, 3:])
