"""CPU tests of the OpenPose clip front end (src/openpose_3dpose_sandbox.py:39-227, 426-433): the
oracle's smoothing against the reference's own read_openpose_json (tests/golden/clip_goldens.npz,
made by tests/golden/make_clip_golden.py), the JSON reader, its errors, and the Maya export."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import clip_oracle  # noqa: E402
import openpose_frontend as of  # noqa: E402

GOLD = os.path.join(HERE, "golden", "clip_goldens.npz")
KEYS = {"coco": "pose_keypoints_2d", "tfpose": "pose_keypoints", "body25": "pose_keypoints_2d"}


@pytest.fixture(scope="module")
def g():
    with np.load(GOLD, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def write_clip(d, raw, key, start=0, skip=()):
    for i, row in enumerate(raw):
        if i in skip:
            continue
        with open(os.path.join(d, "clip_%012d_keypoints.json" % (start + i)), "w") as f:
            json.dump({"people": [{key: [float(v) for v in row]}, {key: [1.0] * len(row)}]}, f)
    with open(os.path.join(d, "notes.txt"), "w") as f:       # (other file types are ignored)
        f.write("not a frame")


def test_goldens_cover_the_cases(g):
    cases = list(g["cases"])
    assert sorted(cases) == sorted("%s_%d" % (f, n) for f in KEYS for n in (9, 10, 23))
    for c in cases:
        xy = g["xy_" + c]
        assert 0.35 < (xy == 0).mean() < 0.6
        assert np.all(xy[:5, 4] == 0) and np.all(xy[-5:, 7] == 0)   # the zero runs (joint 2 x, joint 3 y)


def test_oracle_smooth_equals_reference_bit_for_bit(g):
    for c in g["cases"]:
        got = clip_oracle.smooth(g["xy_" + c])
        np.testing.assert_array_equal(got, g["sm_" + c])
        assert same_bits(got, g["sm_" + c]), c              # (the signs of zeros too)
        assert same_bits(clip_oracle.smooth(g["xy_" + c], smooth=False), g["xy_" + c])


@pytest.mark.parametrize("other_key", [False, True])
def test_read_openpose_json_reproduces_golden_inputs(g, tmp_path, other_key):
    for c in g["cases"]:
        fmt = c.split("_")[0]
        key = KEYS[fmt]
        if other_key:
            key = "pose_keypoints" if key == "pose_keypoints_2d" else "pose_keypoints_2d"
        d = tmp_path / (c + key)
        d.mkdir()
        write_clip(str(d), g["raw_" + c], key)
        numbers, xy = of.read_openpose_json(str(d))
        np.testing.assert_array_equal(numbers, np.arange(len(xy)))
        assert xy.dtype == np.float64 and same_bits(xy, g["xy_" + c]), c
        of.check_clip(numbers)


def test_frame_numbers_and_errors(g, tmp_path):
    raw = g["raw_coco_23"]
    a = tmp_path / "a"
    a.mkdir()
    write_clip(str(a), raw[:12], KEYS["coco"], start=40)     # numbering may start above 0
    numbers, xy = of.read_openpose_json(str(a))
    np.testing.assert_array_equal(numbers, np.arange(40, 52))
    assert same_bits(xy, g["xy_coco_23"][:12])
    of.check_clip(numbers)
    for n in range(2, 9):                                    # 2..8 frames: an error, as the reference
        with pytest.raises(ValueError, match="min 9 frames"):
            of.check_clip(np.arange(n))
        with pytest.raises(ValueError):
            clip_oracle.smooth(np.ones((n, 36)))
        of.check_clip(np.arange(n), smooth=False)
    b = tmp_path / "b"
    b.mkdir()
    write_clip(str(b), raw[:12], KEYS["coco"], skip=(5,))    # a gap in the numbering
    numbers, _ = of.read_openpose_json(str(b))
    assert len(numbers) == 11
    with pytest.raises(ValueError, match="contiguous"):
        of.check_clip(numbers)
    of.check_clip(numbers, smooth=False)
    with pytest.raises(ValueError):
        of.read_openpose_json(str(tmp_path))                 # no frame files


def test_single_file_passes_through(g, tmp_path):
    raw = g["raw_body25_9"][:1]
    write_clip(str(tmp_path), raw, KEYS["body25"], start=7)
    numbers, xy = of.read_openpose_json(str(tmp_path))
    assert list(numbers) == [7] and same_bits(xy, g["xy_body25_9"][:1])
    of.check_clip(numbers)
    assert same_bits(clip_oracle.smooth(xy), xy)


def test_post_oracle_cache_on_fail():
    """The oracle's own post-processing on hand-made rows: zeros / -1 before the first good frame,
    a held run, the -1000 threshold exactly, NaN not failing."""
    rng = np.random.default_rng(5)
    un = rng.uniform(-300, 300, (6, 96))
    xy_s = rng.uniform(400, 700, (6, 36))
    un[0, 0] = -5000.0                                       # frame 0 fails: zeros
    un[3, 3] = -4000.0                                       # frames 3, 4 fail: frame 2 shown
    un[4, 6] = -4000.0
    un[5, 9] = np.nan                                        # NaN minimum: kept
    poses, src = clip_oracle.post(un, xy_s)
    assert list(src) == [-1, 1, 2, 2, 2, 5]
    assert not poses[0].any() and same_bits(poses[3], poses[2]) and same_bits(poses[4], poses[2])
    assert np.isnan(poses[5]).any()
    off, src_off = clip_oracle.post(un, xy_s, cache_on_fail=False)
    assert list(src_off) == list(range(6)) and off[0, 0] == un[0, 0] + (xy_s[0, 2] - 630)
    p = un[1].reshape(32, 3)
    z = p[:, 1]
    np.testing.assert_array_equal(poses[1].reshape(32, 3)[:, 2],
                                  ((max(0.0, z.max()) - z) + min(10000.0, z.min())) + (500 - xy_s[1, 3]))
    np.testing.assert_array_equal(poses[1].reshape(32, 3)[:, 1], p[:, 2])


def test_export_maya_round_trips(tmp_path):
    rng = np.random.default_rng(2)
    poses, xy_s = rng.uniform(-900, 900, (4, 96)), rng.uniform(0, 900, (4, 36))
    numbers = [3, 4, 5, 6]
    p3, p2 = of.export_maya(str(tmp_path / "maya"), numbers, poses, xy_s)
    assert os.path.basename(p3) == "3d_data.json" and os.path.basename(p2) == "2d_data.json"
    three, two = json.load(open(p3)), json.load(open(p2))
    assert sorted(three) == sorted(two) == ["3", "4", "5", "6"]
    for n, frame in enumerate(numbers):
        f3, f2 = three[str(frame)], two[str(frame)]
        assert sorted(f3, key=int) == [str(j) for j in range(32)]
        assert sorted(f2, key=int) == [str(j) for j in range(18)]
        got3 = np.array([f3[str(j)]["translate"] for j in range(32)])
        got2 = np.array([f2[str(j)]["translate"] for j in range(18)])
        assert same_bits(got3.reshape(96), poses[n]) and same_bits(got2.reshape(36), xy_s[n])
        assert list(f3["0"]) == ["translate"]
    with pytest.raises(ValueError):
        of.export_maya(str(tmp_path), numbers, poses[:, :90], xy_s)
