"""Golden vectors for the joints <-> bones conversions, made by calling the REFERENCE's own
``src/top_vae_3d_pose/bones.py`` (get_bones_joints, convert_to_bones, convert_to_joints).

Run in the build container only (the reference is not on the GPU box):

    python tests/golden/make_bones_golden.py

The module imports TensorFlow and the reference's args_def at its top; neither is needed by the
three numpy functions, so both are stubbed in ``sys.modules``.

Output: tests/golden/bones_goldens.npz -- inputs and expected outputs only:

* ``bja``, ``bjb``: what get_bones_joints derives from src/bones_mapping.yml (copied beside this
  file as bones_mapping.yml, a fixture);
* ``joints`` [64, 48] float32: standard-normal rows, rows scaled by 1e-3 and by 1e3, one row with
  two coincident joints (a zero-length bone: a NaN cosine triple) and one all-zero row;
* ``mag`` [64, 16], ``cos`` [64, 48] float32: convert_to_bones(joints);
* ``back`` [64, 48] float64: convert_to_joints of those bones;
* ``free_mag`` [64, 16], ``free_cos`` [64, 48] float32: unconstrained rows, as a decoder gives them
  (neither unit vectors nor non-negative lengths), and ``free_back`` [64, 48] float64 their
  convert_to_joints.
"""
import importlib
import os
import sys
import types

import numpy as np
import yaml

REF = "/root/reference/src"
HERE = os.path.dirname(os.path.abspath(__file__))


class _Anything(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything(name)

    def __call__(self, *a, **k):
        return _Anything("result")


def load_reference():
    for name in ("tensorflow", "top_vae_3d_pose.args_def"):
        sys.modules[name] = _Anything(name)
    pkg = types.ModuleType("top_vae_3d_pose")
    pkg.__path__ = [os.path.join(REF, "top_vae_3d_pose")]
    sys.modules["top_vae_3d_pose"] = pkg
    return importlib.import_module("top_vae_3d_pose.bones")


def main():
    mod = load_reference()
    with open(os.path.join(REF, "bones_mapping.yml")) as f:
        text = f.read()
    mapping = yaml.load(text, Loader=yaml.FullLoader)
    bja, bjb = mod.get_bones_joints(mapping)
    rng = np.random.default_rng(20241020)
    joints = rng.standard_normal((64, 48)).astype(np.float32)
    joints[40:50] *= np.float32(1e-3)
    joints[50:60] *= np.float32(1e3)
    joints[62, 3 * 4:3 * 4 + 3] = joints[62, 3 * 3:3 * 3 + 3]      # joints 5 and 4 coincide: bone 4 has no length
    joints[63] = 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        mag, cos = mod.convert_to_bones(joints, (bja, bjb))
        back = mod.convert_to_joints(mapping, mag, cos.reshape(len(cos), 16, 3))
    free_mag = rng.standard_normal((64, 16)).astype(np.float32)
    free_cos = (1.5 * rng.standard_normal((64, 48))).astype(np.float32)
    free_cos[5, 7] = -0.0
    free_mag[6, 0] = 0.0
    free_back = mod.convert_to_joints(mapping, free_mag, free_cos.reshape(64, 16, 3))
    assert mag.dtype == cos.dtype == np.float32 and back.dtype == free_back.dtype == np.float64
    assert np.isnan(cos[62]).sum() == 3 and np.isnan(cos[63]).all() and not np.isnan(cos[:62]).any()
    path = os.path.join(HERE, "bones_goldens.npz")
    np.savez_compressed(path, bja=np.asarray(bja, np.int64), bjb=np.asarray(bjb, np.int64), joints=joints, mag=mag,
                        cos=cos, back=back, free_mag=free_mag, free_cos=free_cos, free_back=free_back)
    with open(os.path.join(HERE, "bones_mapping.yml"), "w") as f:
        f.write(text)
    print("wrote", path, os.path.getsize(path), "bytes; bja", bja, "bjb", bjb)


if __name__ == "__main__":
    main()
