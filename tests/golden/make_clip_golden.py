"""Golden vectors for the OpenPose clip front end, made by calling the REFERENCE's own
``read_openpose_json`` (src/openpose_3dpose_sandbox.py:39-227).

Run in the build container only (the reference is not on the GPU box):

    python tests/golden/make_clip_golden.py

The sandbox module imports TensorFlow, OpenCV, imageio and the reference's model code at its top;
none of that is needed by ``read_openpose_json``, so those modules are stubbed in ``sys.modules``
and the module's ``plt`` (two curve plots written to ./gif_output) is replaced by a no-op.  The
function is then driven on synthetic directories of OpenPose JSON files:

* three input formats: COCO-18 with confidences (54 values, key ``pose_keypoints_2d``),
  tf-pose-estimation (36 values, key ``pose_keypoints``), body_25 (75 values);
* N in {9, 10, 23} frames, numbered from 0;
* about 45 % of the coordinates zeroed (a few as -0.0), a zero run at the start of one column and
  at the end of another.

Output: tests/golden/clip_goldens.npz -- per case ``raw_*`` [N, L] (the JSON lists), ``xy_*``
[N, 36] (the function's smooth=False result: the parsed frames) and ``sm_*`` [N, 36] (its smoothed
result), inputs and expected outputs only.
"""
import importlib
import json
import os
import sys
import tempfile
import types

import numpy as np

REF = "/root/reference/src"
HERE = os.path.dirname(os.path.abspath(__file__))


class _Anything(types.ModuleType):
    """A module whose every attribute is a harmless callable object."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything(name)

    def __call__(self, *a, **k):
        return _Anything("result")


def load_reference():
    always = ["tensorflow", "cv2", "imageio", "viz", "cameras", "data_utils", "predict_3dpose"]
    maybe = ["matplotlib", "matplotlib.pyplot", "matplotlib.gridspec", "scipy", "scipy.interpolate"]
    for name in always:
        sys.modules[name] = _Anything(name)
    for name in maybe:
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = _Anything(name)
    sys.path.insert(0, REF)
    mod = importlib.import_module("openpose_3dpose_sandbox")
    mod.plt = _Anything("plt")
    return mod


FORMATS = {"coco": (18, True, "pose_keypoints_2d"), "tfpose": (18, False, "pose_keypoints"),
           "body25": (25, True, "pose_keypoints_2d")}


def synth(rng, fmt, n):
    joints, conf, _ = FORMATS[fmt]
    xy = rng.uniform(40.0, 900.0, (n, joints, 2))
    drop = rng.random((n, joints, 2)) < 0.45
    xy[drop] = 0.0
    xy[drop & (rng.random((n, joints, 2)) < 0.1)] = -0.0
    xy[:5, 2, 0] = 0.0                      # a zero run at the start of one column ...
    xy[-5:, 3, 1] = 0.0                     # ... and at the end of another
    if not conf:
        return xy.reshape(n, joints * 2)
    c = rng.uniform(0.1, 1.0, (n, joints, 1))
    return np.concatenate([xy, c], axis=2).reshape(n, joints * 3)


def run(mod, raw, key, smooth):
    with tempfile.TemporaryDirectory() as d:
        for i, row in enumerate(raw):
            with open(os.path.join(d, "clip_%012d_keypoints.json" % i), "w") as f:
                json.dump({"people": [{key: [float(v) for v in row]}]}, f)
        mod.openpose_output_dir = d
        res = mod.read_openpose_json(smooth)
    assert sorted(res) == list(range(len(raw)))
    return np.array([[float(v) for v in res[i]] for i in range(len(raw))], np.float64)


def main():
    mod = load_reference()
    rng = np.random.default_rng(20241019)
    out = {}
    for fmt in FORMATS:
        for n in (9, 10, 23):
            raw = synth(rng, fmt, n)
            name = "%s_%d" % (fmt, n)
            out["raw_" + name] = raw
            out["xy_" + name] = run(mod, raw, FORMATS[fmt][2], False)
            out["sm_" + name] = run(mod, raw, FORMATS[fmt][2], True)
    out["cases"] = np.array(sorted(k[4:] for k in out if k.startswith("raw_")))
    path = os.path.join(HERE, "clip_goldens.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
