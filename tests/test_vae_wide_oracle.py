"""Host-side checks of the wide VAE filter (in > 256; csrc/p3d_vae_wide.h): the shape limits, the LDS
the wide form asks for, the p3d_vae_cat argument errors, the integer cases the GPU tests compare
bit for bit, and the feature-archive reader.  No GPU needed."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _p3d
import vae_exact as ve

HERE = os.path.dirname(os.path.abspath(__file__))
LDS_LIMIT = 160 * 1024
WIDE = (1360, (40, 32), 24, (32, 40), 48)
EDGE264 = (264, (8,), 8, (24,), 48)


def _create(i, enc, lat, dec, out, mb=64):
    e, d = (ctypes.c_int32 * max(len(enc), 1))(*enc), (ctypes.c_int32 * max(len(dec), 1))(*dec)
    h = ctypes.c_void_p()
    rc = _p3d.lib().p3d_vae_create(i, len(enc), e, lat, len(dec), d, out, mb, 1, ctypes.byref(h))
    msg = _p3d.lib().p3d_last_error().decode()
    if rc == 0:
        _p3d.lib().p3d_vae_destroy(h)
    return rc, msg


def _lds(i, enc, lat, dec, out):
    e, d = (ctypes.c_int32 * len(enc))(*enc), (ctypes.c_int32 * len(dec))(*dec)
    return _p3d.lib().p3d_vae_lds_bytes(i, len(enc), e, lat, len(dec), d, out)


def test_wide_shapes_are_accepted_and_the_limits_hold():
    rc, msg = _create(1360, [40, 32], 24, [32, 40], 48)
    assert rc != _p3d.P3D_ERR_ARG, msg
    if not torch.cuda.is_available():
        assert rc == 2, (rc, msg)      # the missing device, as the default shape answers
    for i in (1364, 2056):
        rc, msg = _create(i, [40, 32], 24, [32, 40], 48)
        assert rc == _p3d.P3D_ERR_ARG and "in must" in msg, (i, rc, msg)


def test_wide_lds_and_narrow_lds_unchanged():
    for i in (1360, 264, 2048):
        assert 0 < _lds(i, [40, 32], 24, [32, 40], 48) <= LDS_LIMIT, i
    with open(os.path.join(HERE, "golden", "vae_lds_parent.json")) as f:
        parent = json.load(f)
    assert len(parent) >= 6
    for rec in parent:
        i, enc, lat, dec, out = rec["shape"]
        assert _lds(i, enc, lat, dec, out) == rec["lds_bytes"], rec


def _cat(widths, ptrs, rows=None, idx=None):
    c = _p3d.P3DVaeCat()
    c.n = len(widths)
    for s in range(min(len(widths), 4)):
        c.w[s], c.p[s] = widths[s], ptrs[s]
        c.rows[s] = 100 if rows is None else rows[s]
        c.idx[s] = None if idx is None else idx[s]
    return c


def test_cat_argument_errors_answer_without_a_gpu():
    lib = _p3d.lib()
    A = 0x10000    # (never dereferenced: the checks are pure host code)
    ok = _cat([32, 48, 1280], [A, A, A])
    assert lib.p3d_vae_cat_check(ctypes.byref(ok), 1360, 64) == 0
    bad = [(_cat([], []), "segments"), (_cat([8] * 5, [A] * 5), "segments"),
           (_cat([4, 1356], [A, A]), "multiples of 8"), (_cat([32, 48, 1272], [A, A, A]), "sum to in"),
           (_cat([32, 48, 1280], [A, None, A]), "null segment"), (_cat([32, 48, 1280], [A, A + 4, A]), "aligned"),
           (_cat([32, 48, 1280], [A, A, A], rows=[100, 100, 10]), "needs B rows"),
           (_cat([32, 48, 1280], [A, A, A], rows=[100, 0, 100]), "at least one row")]
    bad[1][0].n = 5
    for c, word in bad:
        assert lib.p3d_vae_cat_check(ctypes.byref(c), 1360, 64) == _p3d.P3D_ERR_ARG, word
        assert word in lib.p3d_last_error().decode(), (word, lib.p3d_last_error().decode())
    # a short table is fine behind an index (the device clamps the index into it)
    assert lib.p3d_vae_cat_check(ctypes.byref(_cat([32, 48, 1280], [A, A, A], rows=[100, 100, 10], idx=[None, None, A])),
                                 1360, 64) == 0
    # the calls themselves: the struct's errors first, then the null filter -- never a GPU
    f3 = (ctypes.c_float * 3)(1, 1, 1)
    for c, word in bad[:3] + bad[4:5]:
        assert lib.p3d_vae_forward_cat(None, ctypes.byref(c), 64, None, 0, None, None, None, None, None, None,
                                       None) == _p3d.P3D_ERR_ARG
        assert word in lib.p3d_last_error().decode()
        assert lib.p3d_vae_train_step_cat(None, ctypes.byref(c), None, 64, None, f3, 1e-3, None, None) == _p3d.P3D_ERR_ARG
        assert word in lib.p3d_last_error().decode()
    for fn in (lib.p3d_vae_loss_cat, lib.p3d_vae_grad_cat):
        assert fn(None, ctypes.byref(ok), None, 64, None, 0, f3, None, None) == _p3d.P3D_ERR_ARG
        assert "null argument" in lib.p3d_last_error().decode()
        assert fn(None, None, None, 64, None, 0, f3, None, None) == _p3d.P3D_ERR_ARG


@pytest.mark.parametrize("B", (16, 64, 128))
@pytest.mark.parametrize("shape", (WIDE, EDGE264), ids=("wide", "edge264"))
def test_integer_cases_prove_themselves_exact(shape, B):
    k = ve.exact_case(B, shape)
    assert max(k["worst"].values()) < ve.LIMIT
    assert k["grads"]["enc_h_%d/kernel" % shape[1][0]].shape == (shape[0], shape[1][0])


def _feature_archive(path, keys, sizes, extra=3, width=16, drop=None, short=None):
    rng = np.random.default_rng(4)
    members = {}
    for (subj, act, name), n in zip(keys, sizes):
        rows = n + extra if (subj, act, name) != short else n - 1
        if (subj, act, name) != drop:
            members["%s/%s/%s/data" % (subj, act, name.replace(".h5", ""))] = \
                (0.1 * rng.standard_normal((rows, width))).astype(np.float32)
    np.savez(path, **members)
    return members


def test_load_effnet_outputs(tmp_path):
    from top_vae_3d_pose import data_handler
    keys = [(9, "Walking", "Walking 1.54138969.h5"), (1, "Directions", "Directions.60457274.h5"),
            (1, "Walking", "Walking.55011271.h5")]
    sizes = [7, 5, 9]
    path = str(tmp_path / "effnet.npz")
    members = _feature_archive(path, keys, sizes)
    out = data_handler.load_effnet_outputs(path, keys, sizes)
    assert out.shape == (21, 16) and out.dtype == np.float32
    ref = np.concatenate([members["%s/%s/%s/data" % (s, a, n.replace(".h5", ""))][:z] for (s, a, n), z in zip(keys, sizes)])
    np.testing.assert_array_equal(out, ref)
    # the key order is the caller's, not the archive's
    out2 = data_handler.load_effnet_outputs(path, keys[::-1], sizes[::-1])
    np.testing.assert_array_equal(out2[:9], ref[12:])
    _feature_archive(path, keys, sizes, drop=keys[1])
    with pytest.raises(ValueError, match="Directions"):
        data_handler.load_effnet_outputs(path, keys, sizes)
    _feature_archive(path, keys, sizes, short=keys[2])
    with pytest.raises(ValueError, match="Walking.55011271"):
        data_handler.load_effnet_outputs(path, keys, sizes)


def test_effnet_flags_follow_the_reference():
    from top_vae_3d_pose.args_def import ENVIRON as ENV
    f = ENV.setup(argv=[])
    assert f.effnet_outputs_path == "data/human36m_effnet.hdf5" and f.use_effb1 is False
    f = ENV.setup(argv=["--use_effb1", "--effnet_outputs_path", "x.npz"])
    assert f.use_effb1 and f.effnet_outputs_path == "x.npz"
    ENV.setup(argv=[])
