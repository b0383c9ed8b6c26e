"""The rigid skeleton's definitions checked on the numpy oracle (tests/skel_oracle.py)
against what they must mean: the composed rotations turn the rest directions into the bones'
directions, forward kinematics reproduces the rigid pose, the Euler angles rebuild the rotation
matrices (also through scipy, where present), and a BVH file written by
openpose_frontend.export_bvh and read back by a reader that shares nothing with the writer gives
the rigid pose again.  No GPU, no library.

Tolerance 1e-9 max(1, |value|): unit roundoff 1.1e-16, the longest chain has 6 bones of a few dozen
operations each plus a handful of few-ulp libm calls -- order 1e-13 relative; a wrong sign, axis or
order is off by order 1."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import openpose_frontend as of  # noqa: E402
import skel_oracle as so  # noqa: E402

N = 96


@pytest.fixture(scope="module")
def clip():
    """Random rows (every bone away from the antiparallel branch), their lengths and pose."""
    rng = np.random.default_rng(11)
    poses = so.random_rows(rng, N)
    off = np.array([0, N])
    L, used = so.lengths(poses, None, off)
    return dict(poses=poses, off=off, L=L, used=used, **so.pose(poses, None, off, L))


def special_rows():
    """Rows with, per row, bones exactly antiparallel to their rest direction, bones of zero length
    and gimbal poses (the spine straight along +-Z: R21 = +-1), the rest random."""
    rng = np.random.default_rng(12)
    n = 8
    d, ln = so.random_directions(rng, n), rng.uniform(50.0, 500.0, (n, 16))
    anti, zero = [(0, 0), (0, 9), (1, 4), (1, 5), (2, 12), (3, 6), (3, 7)], [(4, 0), (4, 1), (5, 8), (5, 15), (6, 10)]
    for f, b in anti:
        d[f, b] = -so.REST[b]
    for f, b in zero:
        ln[f, b] = 0.0
    d[6, 6], d[7, 6] = (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)
    return so.rows_from(rng.uniform(-1000.0, 1000.0, (n, 3)), d, ln), anti, zero


def check_a_b(poses, L, out):
    J = so.to_skeleton(poses)
    d, _ = so.directions(J)
    g = so.composed(out["quat"])
    so.close(so.rotate(g, so.REST[None]), d, "(a) the composed rotation takes r_b to d_b")
    so.close(np.linalg.norm(out["quat"], axis=-1), np.ones(out["quat"].shape[:2]), "unit quaternions")
    for s, (a, b) in enumerate(zip([0], [len(poses)])):
        so.close(so.fk(out["root"][a:b], L[s], out["quat"][a:b]), out["rigid"][a:b], "(b) forward kinematics")
    so.close(out["rigid"][:, 0], J[:, 0], "the rigid pose starts at the hip")


def test_generated_rows_stay_clear_of_the_antiparallel_branch(clip):
    m = so.margins(clip["poses"])
    assert m.shape == (N, 16) and (m >= so.MARGIN).all()
    assert np.isnan(clip["poses"]).any()                      # the joints the skeleton does not use: ignored
    assert clip["used"][0] == N and np.isfinite(clip["L"]).all()
    assert ((clip["L"] > 50.0) & (clip["L"] < 500.0)).all()


def test_a_b_rotations_and_forward_kinematics(clip):
    check_a_b(clip["poses"], clip["L"], clip)
    # with the frame's own lengths the rigid pose is the pose
    J = so.to_skeleton(clip["poses"])
    _, ln = so.bones(J)
    for f in range(4):
        own = so.pose(clip["poses"][f:f + 1], None, np.array([0, 1]), ln[f:f + 1])
        so.close(own["rigid"], J[f:f + 1], "rigid pose with the frame's own lengths")


def test_c_euler_angles_rebuild_the_matrices(clip):
    so.close(so.euler_matrix(clip["euler"]), so.quat_matrix(clip["quat"]), "(c) Rz Rx Ry of the Euler triple")
    poses, _, _ = special_rows()
    out = so.pose(poses, None, np.array([0, len(poses)]), np.full((1, 16), 100.0))
    R = so.quat_matrix(out["quat"])
    assert abs(R[6, 6, 2, 1] - 1.0) < 1e-15 and abs(R[7, 6, 2, 1] + 1.0) < 1e-15      # the gimbal rows: R21 = +-1
    assert np.hypot(R[6:8, 6, 0, 1], R[6:8, 6, 1, 1]).max() < 1e-12
    assert (out["euler"][6:8, 6, 2] == 0.0).all() and np.allclose(out["euler"][6:8, 6, 1], [90.0, -90.0], atol=1e-6)
    so.close(so.euler_matrix(out["euler"]), R, "(c) on the special rows")


def test_d_scipy_agrees_on_the_conventions(clip):
    pytest.importorskip("scipy")
    from scipy.spatial.transform import Rotation
    e, q = clip["euler"].reshape(-1, 3), clip["quat"].reshape(-1, 4)
    by_euler = Rotation.from_euler("ZXY", e, degrees=True).as_matrix()
    by_quat = Rotation.from_quat(q[:, [1, 2, 3, 0]]).as_matrix()
    so.close(by_euler, by_quat, "(d) scipy: ZXY Euler against the quaternion")
    so.close(by_euler, so.quat_matrix(q), "(d) scipy against the oracle's matrix")


def test_e_bvh_written_and_read_back(clip, tmp_path):
    path = of.export_bvh(str(tmp_path / "clip" / "skeleton.bvh"), np.arange(5, 5 + N), clip["L"][0], clip["euler"],
                         clip["root"], fps=25.0)
    nodes, frame_time, motion = so.read_bvh(path)
    assert motion.shape == (N, 6 + 16 * 3) and frame_time == 1.0 / 25.0
    assert (motion[:, 3:6] == 0.0).all()                                          # the root never rotates
    so.close(so.bvh_rigid(so.bvh_positions(nodes, motion)), clip["rigid"], "(e) forward kinematics from the file's text")
    # the hierarchy, restated by the oracle: names, parents and offsets
    assert nodes[0][:2] == ("Hips", -1) and not nodes[0][2].any()
    assert nodes[0][3] == ["Xposition", "Yposition", "Zposition", "Zrotation", "Xrotation", "Yrotation"]
    got = {n[0]: (nodes[n[1]][0], n[2], n[3]) for n in nodes[1:]}
    want = so.hierarchy(clip["L"][0])
    assert len(want) == len(got) == 16 + 5
    for name, parent, offset in want:
        assert got[name][0] == parent and got[name][1].tobytes() == offset.tobytes(), name
        assert got[name][2] == ([] if name.startswith("End_") else ["Zrotation", "Xrotation", "Yrotation"])
    text = open(path).read()
    assert text.count("JOINT bone_") == 16 and text.count("End Site") == 5 and "Frames: %d\n" % N in text
    assert repr(float(clip["euler"][3, 7, 1])) in text.splitlines()[-N + 3].split()   # repr precision


def test_f_antiparallel_and_zero_length_bones():
    poses, anti, zero = special_rows()
    off = np.array([0, len(poses)])
    L = np.random.default_rng(13).uniform(50.0, 500.0, (1, 16))
    out = so.pose(poses, None, off, L)
    m = so.margins(poses)
    g = so.composed(out["quat"])
    for f, b in anti:
        assert m[f, b] == 0.0
        so.close(g[f, b], [0.0, 0.0, 0.0, 1.0], "half a turn about Z")
    _, zl = so.directions(so.to_skeleton(poses))
    assert sorted(zip(*np.nonzero(zl))) == sorted(zero)
    for f, b in zero:
        so.close(g[f, b], [1.0, 0.0, 0.0, 0.0], "a zero-length bone is the identity")
    check_a_b(poses, L, out)
    so.close(so.euler_matrix(out["euler"]), so.quat_matrix(out["quat"]), "(c) on the special rows")


def test_lengths_count_only_frames_with_their_own_finite_pose():
    rng = np.random.default_rng(14)
    poses = so.random_rows(rng, 12)
    off = np.array([0, 5, 9, 12])
    src = np.arange(12)
    src[1], src[2] = 0, 0                                   # held duplicates
    src[5:9] = -1                                           # a clip of zero rows
    poses[5:9] = 0.0
    poses[10, 3 * 13] = np.nan                              # one NaN joint (Thorax)
    L, used = so.lengths(poses, src, off)
    assert used.tolist() == [3, 0, 2] and not L[1].any()
    _, ln = so.bones(so.to_skeleton(poses))
    so.close(L[0], ln[[0, 3, 4]].mean(axis=0), "clip 0")
    so.close(L[2], ln[[9, 11]].mean(axis=0), "clip 2")
    out = so.pose(poses, src, off, L)
    assert (out["quat"][5:9] == [1.0, 0.0, 0.0, 0.0]).all() and not out["euler"][5:9].any()   # zero rows: the identity
    # the NaN joint (skeleton joint 8): bones 7 and 8 touch it, their children's local rotations follow
    bad = np.isnan(out["quat"][10]).any(axis=-1)
    assert bad.tolist() == [b in (7, 8, 9, 10, 13) for b in range(16)]
    assert np.isfinite(out["quat"][[9, 11]]).all()


def test_export_bvh_refusals(clip, tmp_path):
    args = (np.arange(N), clip["L"][0], clip["euler"], clip["root"])
    with pytest.raises(ValueError, match="zero.bvh.*n_used == 0"):
        of.export_bvh(str(tmp_path / "zero.bvh"), args[0], np.zeros(16), *args[2:])
    e = clip["euler"].copy()
    e[2, 3, 1] = np.nan
    with pytest.raises(ValueError, match="nan.bvh.*non-finite"):
        of.export_bvh(str(tmp_path / "nan.bvh"), args[0], args[1], e, args[3])
    with pytest.raises(ValueError):
        of.export_bvh(str(tmp_path / "short.bvh"), args[0][:-1], *args[1:])
    with pytest.raises(ValueError, match="fps"):
        of.export_bvh(str(tmp_path / "fps.bvh"), *args, fps=0.0)
    with pytest.raises(ValueError):
        of.export_bvh_clips(str(tmp_path), ["a", "b"], [args[0]], [dict(lengths=args[1], euler=args[2], root=args[3])])
    paths = of.export_bvh_clips(str(tmp_path / "out"), ["a"], [args[0]], [dict(lengths=args[1], euler=args[2], root=args[3])])
    assert paths == [str(tmp_path / "out" / "a" / "skeleton.bvh")] and os.path.exists(paths[0])
    assert not os.path.exists(str(tmp_path / "zero.bvh"))
