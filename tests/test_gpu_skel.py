"""Lifted rows as a rigid skeleton on the GPU (include/p3d.h: p3d_skel_lengths / p3d_skel_pose;
ClipLifter.skeleton, skeleton_rows, export_bvh) against tests/skel_oracle.py, which states the same
float64 operations in numpy.

Tolerances: lengths 1e-9 relative (the mean of at most 2^20 positive terms loses at most N u, about
1.2e-10); quat, euler, rigid and root 1e-9 max(1, |value|) (unit roundoff 1.1e-16, the longest chain
has 6 bones of a few dozen operations each plus a handful of few-ulp libm calls: order 1e-13
relative).  Everything said to be the same bits is compared as bytes."""
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
import linear_model  # noqa: E402
import openpose_frontend as of  # noqa: E402
import skel_oracle as so  # noqa: E402
import test_gpu_clip as tc  # noqa: E402  (clip_for_model, USE2, IGN3, GOLD, assert_same_bits)
from oracle import ref_mlp  # noqa: E402

C = int(_p3d.lib().p3d_skel_chunk())
OUTS = (("quat", 64), ("euler", 48), ("rigid", 51), ("root", 3))            # doubles per row
GUARD, SENTINEL = 64, -7.0                              # guard words around every output (float64 and int64 alike)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def run(poses, src, off, lengths=None, want=("quat", "euler", "rigid", "root"), off_dev=None):
    """The two calls (p3d_skel_lengths unless lengths are passed in [S, 16]) on fresh buffers with
    guard words around every output -> dict(L, used, quat, euler, rigid, root as asked for)."""
    lib, p = _p3d.lib(), _p3d.ptr
    off = np.ascontiguousarray(off, np.int64)
    S, N = len(off) - 1, int(off[-1])
    d_poses = torch.from_numpy(np.ascontiguousarray(poses, np.float64)).cuda()
    d_src = None if src is None else torch.from_numpy(np.asarray(src, np.int32)).cuda()
    d_off = torch.from_numpy(off if off_dev is None else np.ascontiguousarray(off_dev, np.int64)).cuda()
    guarded = lambda n, dt=torch.float64: torch.full((n + 2 * GUARD,), SENTINEL, dtype=dt, device="cuda")   # noqa: E731
    bufs = {k: guarded(N * w) for k, w in OUTS if k in want}
    bufs["L"], d_used = guarded(S * 16), guarded(S, torch.int64)
    ptr = lambda t: p(t) + GUARD * 8   # noqa: E731
    nbytes = int(lib.p3d_skel_workspace(N, S))
    work = torch.full((nbytes // 8 + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    st = _p3d.stream_handle()
    if lengths is None:
        _p3d.check(lib.p3d_skel_lengths(p(d_poses), p(d_src), off.ctypes.data, p(d_off), S, N, ptr(bufs["L"]), ptr(d_used),
                                        ptr(work), nbytes, st), "p3d_skel_lengths")
    else:
        bufs["L"][GUARD:GUARD + S * 16] = torch.from_numpy(np.ascontiguousarray(lengths, np.float64).reshape(-1)).cuda()
    _p3d.check(lib.p3d_skel_pose(p(d_poses), p(d_src), off.ctypes.data, p(d_off), S, N, ptr(bufs["L"]),
                                 *(ptr(bufs[k]) if k in want else None for k, _ in OUTS), st), "p3d_skel_pose")
    torch.cuda.synchronize()
    out = {}
    for k, t in list(bufs.items()) + [("used", d_used), ("work", work)]:
        h = t.cpu().numpy()
        assert (h[:GUARD] == SENTINEL).all() and (h[-GUARD:] == SENTINEL).all(), "%s: a guard word changed" % k
        out[k] = h[GUARD:-GUARD]
    del out["work"]
    shapes = dict(quat=(N, 16, 4), euler=(N, 16, 3), rigid=(N, 17, 3), root=(N, 3), L=(S, 16), used=(S,))
    out = {k: v.reshape(shapes[k]) for k, v in out.items()}
    if lengths is not None:
        del out["used"]
    return out


def check_against_oracle(got, poses, src, off, lengths=None, what=""):
    L, used = so.lengths(poses, src, off)
    if lengths is None:
        np.testing.assert_array_equal(got["used"], used)
        err = np.abs(got["L"] - L) / np.maximum(L, 1e-300)
        assert (err[L > 0] <= 1e-9).all() and (got["L"][L == 0] == 0).all(), "%s lengths off by %.3e" % (what, err.max())
    want = so.pose(poses, src, off, got["L"])                # (the rigid pose from the lengths the kernel used)
    for k, _ in OUTS:
        so.close(got[k], want[k], "%s %s" % (what, k))


@pytest.mark.parametrize("n", [1, 9, 17, C - 1, C, C + 1, 2 * C + 3])
def test_single_clip_matches_the_oracle(n):
    poses = so.random_rows(np.random.default_rng(100 + n), n)
    assert (so.margins(poses) >= so.MARGIN).all()            # no bone near the antiparallel branch: nothing left out
    off = offsets([n])
    got = run(poses, np.arange(n), off)
    assert got["used"][0] == n
    check_against_oracle(got, poses, None, off, what="%d frames" % n)
    again = run(poses, np.arange(n), off)
    for k in got:
        assert same(got[k], again[k]), "%s differs between two identical calls" % k
    assert same(run(poses, None, off)["quat"], got["quat"])   # a null src: every row its own


def test_batch_carries_the_single_clip_bits_and_wrong_offsets_stay_inside():
    lens = [1, 9, C + 1, 300]
    off, N = offsets(lens), sum(lens)
    poses = so.random_rows(np.random.default_rng(7), N)
    src = np.arange(N)
    got = run(poses, src, off)
    check_against_oracle(got, poses, src, off, what="batch")
    for s, (a, b) in enumerate(zip(off[:-1], off[1:])):
        one = run(poses[a:b], np.arange(b - a), offsets([b - a]))
        assert same(one["L"][0], got["L"][s]) and one["used"][0] == got["used"][s] == b - a, "lengths of clip %d" % s
        for k, _ in OUTS:
            assert same(one[k], got[k][a:b]), "%s of clip %d (%d frames)" % (k, s, b - a)
    # a wrong device copy of the offsets changes rows only: the guards (checked in run) are unchanged
    for wrong in ([0, 5, 3, N + 900, N], [-40, 1 << 40, -1, 7, 2], [N, N, N, N, N], [0, 0, 0, 0, 0], [0, N, N, N, N]):
        out = run(poses, src, off, off_dev=wrong)
        assert out["quat"].shape == (N, 16, 4)


def test_special_rows():
    rng = np.random.default_rng(21)
    lens = [C + 5, 6, 20, 11]
    off, N = offsets(lens), sum(lens)
    poses = so.random_rows(rng, N)
    src = np.arange(N)
    held = [3, 4, C - 1, C, C + 1]                           # held duplicates, over a chunk boundary too
    for n in held:
        src[n] = src[n - 1]
        poses[n] = poses[src[n]]
    a1, b1 = off[1], off[2]
    src[a1:b1], poses[a1:b1] = -1, 0.0                       # a clip of zero rows: no counting frame
    z = off[2] + 4
    src[z], poses[z] = -1, 0.0                               # a zero row inside a clip
    nan = off[3] + 2
    poses[nan, 3 * 13 + 1] = np.nan                          # one NaN joint: the thorax (skeleton joint 8)
    got = run(poses, src, off)
    check_against_oracle(got, poses, src, off, what="special rows")
    assert got["used"].tolist() == [lens[0] - len(held), 0, lens[2] - 1, lens[3] - 1]
    assert not got["L"][1].any() and (got["L"][[0, 2, 3]] > 0).all()
    _, ln = so.bones(so.to_skeleton(poses))
    keep = np.setdiff1d(np.arange(off[1]), held)
    so.close(got["L"][0], ln[keep].mean(axis=0), "held rows do not count")
    for n in list(range(a1, b1)) + [z]:                      # zero rows: identity rotations, the rest pose at the origin
        assert (got["quat"][n] == [1.0, 0.0, 0.0, 0.0]).all() and not got["euler"][n].any() and not got["root"][n].any()
    for n in held:
        assert same(got["quat"][n], got["quat"][n - 1])
    bad = np.isnan(got["quat"][nan]).any(axis=-1)
    assert bad.tolist() == [b in (7, 8, 9, 10, 13) for b in range(16)]       # the bones at the joint and their children
    assert np.isnan(got["euler"][nan]).any(axis=-1).tolist() == bad.tolist()
    assert np.isfinite(got["quat"][[nan - 1, nan + 1]]).all() and np.isfinite(got["L"]).all()
    # a zero row whose buffer holds something else still counts as zeros
    junk = poses.copy()
    junk[z] = rng.uniform(-500.0, 500.0, 96)
    assert same(run(junk, src, off)["quat"], got["quat"])
    # lengths passed in are used as given
    given = rng.uniform(50.0, 500.0, (len(lens), 16))
    out = run(poses, src, off, lengths=given)
    assert same(out["L"], given)
    check_against_oracle(out, poses, src, off, lengths=given, what="given lengths")
    assert same(out["quat"], got["quat"]) and not same(out["rigid"], got["rigid"])
    # antiparallel, zero-length and gimbal bones (tests/test_skel_oracle.py's rows)
    import test_skel_oracle as tso
    sp, anti, zero = tso.special_rows()
    out = run(sp, None, offsets([len(sp)]), lengths=given[:1])
    check_against_oracle(out, sp, None, offsets([len(sp)]), lengths=given[:1], what="antiparallel / zero-length / gimbal")
    g = so.composed(out["quat"])
    for f, b in anti:
        so.close(g[f, b], [0.0, 0.0, 0.0, 1.0], "half a turn about Z")
    for f, b in zero:
        so.close(g[f, b], [1.0, 0.0, 0.0, 0.0], "a zero-length bone")


def test_each_output_alone_gives_the_same_bits():
    lens = [C + 3, 17]
    off, N = offsets(lens), sum(lens)
    poses = so.random_rows(np.random.default_rng(33), N)
    src = np.arange(N)
    src[5] = 4
    poses[5] = poses[4]
    both = run(poses, src, off)
    for k, _ in OUTS:
        alone = run(poses, src, off, want=(k,))
        assert sorted(alone) == sorted(["L", "used", k])
        assert same(alone[k], both[k]), "%s on its own" % k
    pair = run(poses, src, off, want=("euler", "root"))
    assert same(pair["euler"], both["euler"]) and same(pair["root"], both["root"])


def test_skeleton_rows_takes_the_lifters_local_src():
    lens = [12, 9]
    off, N = offsets(lens), sum(lens)
    poses = so.random_rows(np.random.default_rng(44), N)
    local = np.concatenate([np.arange(n) for n in lens]).astype(np.int32)
    local[13], poses[13] = -1, 0.0                           # clip 1, position 1: zeros
    local[15], poses[15] = 2, poses[14]                      # clip 1, position 3 shows position 2
    glob = np.where(local >= 0, local + np.repeat(off[:-1], lens), -1)
    res = of.skeleton_rows(poses, local, off)
    want = run(poses, glob, off)
    assert [r["n_used"] for r in res] == want["used"].tolist() == [12, 7]
    for s, r in enumerate(res):
        assert sorted(r) == ["euler", "lengths", "n_used", "quat", "rigid", "root"]
        assert same(r["lengths"], want["L"][s])
        for k, _ in OUTS:
            assert same(r[k], want[k][off[s]:off[s + 1]]), k
    one = of.skeleton_rows(poses[:12], None, [0, 12], lengths=np.full(16, 100.0))[0]
    assert (one["lengths"] == 100.0).all() and one["n_used"] == 12 and same(one["quat"], res[0]["quat"])
    for bad in (dict(poses=poses[:, :95]), dict(offsets=[0, 5]), dict(offsets=[0, 0, N]), dict(src=local[:-1]),
                dict(lengths=np.ones(15)), dict(lengths=-np.ones(16))):
        kw = dict(dict(poses=poses, src=local, offsets=off), **bad)
        with pytest.raises(ValueError):
            of.skeleton_rows(kw.pop("poses"), kw.pop("src"), kw.pop("offsets"), **kw)


# ---- end to end ---------------------------------------------------------------------------------
def small_model():
    """A LinearModel at cfg1's shape (256 wide, one block) and statistics as test_gpu_clip.model_setup
    builds them, the 3D ones narrow: with |mean| <= 200 and std <= 30 every exported value of a
    fresh network stays far above -1000 except the one x that the network does not predict, which
    sits at -900 -- so a frame fails (x + spine_x - 630 < -1000) exactly where its smoothed
    spine_x is below 530, as clip_for_model places them."""
    rng = np.random.default_rng(3)
    st = ref_mlp.init_state(ref_mlp.Cfg(linear_size=256, num_layers=1, residual=True, batch_norm=True), seed=3, bn_seed=4)
    m = linear_model.LinearModel(256, 1, True, True, False, 64, 1e-3, "/tmp/p3d_skel", seed=11)
    m.set_weights({**st.params, **st.moving})
    s = dict(mean2=rng.uniform(200, 600, 64), std2=rng.uniform(50, 150, 64), mean3=rng.uniform(-200, 200, 96),
             std3=rng.uniform(5, 30, 96))
    s["mean3"][int([d for d in tc.IGN3 if d % 3 == 0][0])] = -900.0
    return m, s


def test_lift_clips_then_skeleton_then_bvh(tmp_path):
    m, s = small_model()
    lens = [23, 1, C + 9, 9]
    clips = [tc.clip_for_model(n, 60 + n) for n in lens]
    clips[1][0, 2] = 600.0                                   # the one-frame clip: a good frame
    cl = of.ClipLifter(m, s["mean2"], s["std2"], tc.USE2, s["mean3"], s["std3"], tc.IGN3, max_frames=sum(lens))
    with pytest.raises(ValueError, match="no lift"):
        cl.skeleton()
    res = cl.lift_clips(clips)
    sk = cl.skeleton()
    off = offsets(lens)
    poses = np.concatenate([r["poses"] for r in res])
    local = np.concatenate([r["src"] for r in res])
    position = np.concatenate([np.arange(n) for n in lens])
    assert (local == -1).any() and ((local >= 0) & (local != position)).any()      # zero rows and held rows are there
    rows = of.skeleton_rows(poses, local, off)               # the same calls from the host rows
    glob = np.where(local >= 0, local + np.repeat(off[:-1], lens), -1)
    L, used = so.lengths(poses, glob, off)
    want = so.pose(poses, glob, off, np.array([k["lengths"] for k in sk]))
    for c, (k, r) in enumerate(zip(sk, rows)):
        assert k["n_used"] == used[c] > 0
        so.close(k["lengths"], L[c], "lengths of clip %d" % c)
        for key in ("lengths", "quat", "euler", "rigid", "root"):
            assert same(k[key], r[key]), key
            if key != "lengths":
                so.close(k[key], want[key][off[c]:off[c + 1]], "%s of clip %d" % (key, c))
    names = ["clip%d" % c for c in range(len(lens))]
    numbers = [np.arange(n) for n in lens]
    paths = of.export_bvh_clips(str(tmp_path), names, numbers, sk, fps=30.0)
    for c, path in enumerate(paths):
        assert path == str(tmp_path / names[c] / "skeleton.bvh")
        nodes, ft, motion = so.read_bvh(path)
        assert motion.shape[0] == lens[c] and ft == 1.0 / 30.0
        so.close(so.bvh_rigid(so.bvh_positions(nodes, motion)), sk[c]["rigid"], "the BVH of clip %d read back" % c)
    # a single clip; lengths of a known actor
    p1, _, s1 = cl.lift_clip(clips[0])
    one = cl.skeleton()
    assert len(one) == 1 and same(one[0]["quat"], sk[0]["quat"]) and same(one[0]["lengths"], sk[0]["lengths"])
    given = cl.skeleton(lengths=np.full(16, 123.0))[0]
    assert (given["lengths"] == 123.0).all() and same(given["euler"], one[0]["euler"]) and given["n_used"] == one[0]["n_used"]
    m.check_errors()
    m.close()


def write_clip(d, raw):
    os.makedirs(d, exist_ok=True)
    for i, row in enumerate(raw):
        with open(os.path.join(d, "clip_%012d_keypoints.json" % i), "w") as fh:
            json.dump({"people": [{"pose_keypoints_2d": [float(v) for v in row]}]}, fh)


def tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def driver_frames(rng, n):
    """n frames of 18 plain x / y pairs, no dropped joint, the neck (the sandbox's spine columns)
    at x in 600..800 and y in 100..300."""
    xy = rng.uniform(300.0, 800.0, (n, 36))
    xy[:, 2], xy[:, 3] = rng.uniform(600.0, 800.0, n), rng.uniform(100.0, 300.0, n)
    return xy


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """Two clips of frame files and the drivers' flags for a checkpoint whose output layer is a
    fresh one scaled by 0.002: every pose stays within a few millimetres of the synthetic 3D mean
    (|mean| <= 500), so with the spine columns of driver_frames no exported value comes near -1000
    and every frame carries its own pose.  (A fresh network on the synthetic statistics fails every
    frame: all-zero poses, which --export_bvh refuses.)"""
    import predict_3dpose as p3
    tmp = tmp_path_factory.mktemp("skel_driver")
    rng = np.random.default_rng(5)
    names = {"a_nine": 9, "b_twelve": 12}
    root = tmp / "clips"
    for name, n in names.items():
        write_clip(str(root / name), driver_frames(rng, n))
    base = ["--synthetic", "--residual", "--batch_norm", "--linear_size", "256", "--num_layers", "1", "--max_batch", "128",
            "--verbose", "0", "--train_dir", str(tmp / "train")]
    flags = p3.build_parser().parse_args(base)
    m = p3.create_model(None, ["All"], 128, flags)
    st = m.get_state()
    m.close()
    for k in st:
        if k.endswith(("/w4", "/b4")):
            st[k] = st[k] * np.float32(0.002)
    os.makedirs(p3.train_dir_for(flags), exist_ok=True)
    np.savez(os.path.join(p3.train_dir_for(flags), "checkpoint-1.npz"), **st)
    return root, names, base + ["--load", "1"]


def bvh_against_its_json(bvh, three, n, fps, what):
    """A driver's skeleton.bvh read back against the skeleton of the 3d_data.json beside it."""
    nodes, ft, motion = so.read_bvh(bvh)
    assert motion.shape == (n, 54) and ft == 1.0 / fps
    data = json.load(open(three))
    poses = np.array([[data[str(i)][str(j)]["translate"] for j in range(32)] for i in range(n)]).reshape(n, 96)
    assert poses.any(axis=1).all()                           # no zero row: every frame carries its own pose
    sk = of.skeleton_rows(poses, None, [0, n])[0]
    assert sk["n_used"] == n
    so.close(so.bvh_rigid(so.bvh_positions(nodes, motion)), sk["rigid"], what)


def test_sandbox_driver_export_bvh(driver, tmp_path):
    import openpose_3dpose_sandbox as sandbox
    root, names, base = driver
    plain = sandbox.main(base + ["--clips_root", str(root), "--out_dir", str(tmp_path / "plain")])
    assert tree(str(tmp_path / "plain")) == sorted(os.path.join(n, f) for n in names for f in ("2d_data.json", "3d_data.json"))
    assert all(len(q) == 2 for q in plain)                   # without the flag: the files and paths of before
    with_bvh = sandbox.main(base + ["--clips_root", str(root), "--out_dir", str(tmp_path / "bvh"), "--export_bvh",
                                    "--bvh_fps", "24"])
    assert tree(str(tmp_path / "bvh")) == sorted(os.path.join(n, f) for n in names
                                                  for f in ("2d_data.json", "3d_data.json", "skeleton.bvh"))
    for (name, n), q, w in zip(names.items(), plain, with_bvh):
        assert w[2] == str(tmp_path / "bvh" / name / "skeleton.bvh")
        for a, b in zip(q, w[:2]):                           # the flag changes nothing else
            assert open(a, "rb").read() == open(b, "rb").read()
        bvh_against_its_json(w[2], w[0], n, 24.0, "the BVH of %s against its 3d_data.json" % name)
    one = sandbox.main(base + ["--pose_estimation_json", str(root / "b_twelve"), "--out_dir", str(tmp_path / "one"),
                               "--export_bvh"])
    assert [os.path.basename(q) for q in one] == ["3d_data.json", "2d_data.json", "skeleton.bvh"]
    assert tree(str(tmp_path / "one")) == ["2d_data.json", "3d_data.json", "skeleton.bvh"]
    assert open(one[2]).read().replace(repr(1.0 / 30.0), repr(1.0 / 24.0)) == open(with_bvh[1][2]).read()


def test_realtime_driver_export_bvh(driver, tmp_path):
    import openpose_3dpose_sandbox_realtime as rt
    root, names, base = driver
    live = base + ["--pose_estimation_json", str(root / "b_twelve"), "--idle_exit", "0"]
    plain = rt.main(live + ["--out_dir", str(tmp_path / "plain")])
    assert len(plain) == 2 and tree(str(tmp_path / "plain")) == ["2d_data.json", "3d_data.json"]
    got = rt.main(live + ["--out_dir", str(tmp_path / "bvh"), "--export_bvh", "--bvh_fps", "60"])
    assert [os.path.basename(q) for q in got] == ["3d_data.json", "2d_data.json", "skeleton.bvh"]
    assert tree(str(tmp_path / "bvh")) == ["2d_data.json", "3d_data.json", "skeleton.bvh"]
    for a, b in zip(plain, got[:2]):                         # the flag changes nothing else
        assert open(a, "rb").read() == open(b, "rb").read()
    bvh_against_its_json(got[2], got[0], 12, 60.0, "the live stream's BVH against its 3d_data.json")
