"""Host half of sample() (predict_3dpose.py, src/predict_3dpose.py:447-612): p3d_sample_world's
argument errors (which answer without a GPU), the 2D -> 3D key map, the camera lookup by name,
the rows the reference draws, and the --sample_dir flag."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
LIB = os.path.join(ROOT, "3d-pose-baseline_amd", "libp3d.so")

import sample_oracle as so  # noqa: E402
from synth_cameras import synth_cameras  # noqa: E402


def test_sample_world_argument_errors_without_a_gpu():
    if not os.path.exists(LIB):
        pytest.skip("libp3d.so not built")
    import _p3d
    lib, E = _p3d.lib(), _p3d.P3D_ERR_ARG
    F32, F64, BF16 = _p3d.P3D_DTYPE_F32, _p3d.P3D_DTYPE_F64, _p3d.P3D_DTYPE_BF16
    buf = (ctypes.c_double * 4096)()
    a = ctypes.addressof(buf)
    a += (-a) % 16
    p = lambda off: ctypes.c_void_p(a + off)   # noqa: E731
    good = dict(yn=p(0), in_dtype=F32, N=8, U=48, mean=p(4096), std=p(8192), use=p(12288), root=None,
                cams=p(16384), C=4, cam_of_row=None, out=p(20480))

    def call(word, **kw):
        v = dict(good, **kw)
        rc = lib.p3d_sample_world(v["yn"], v["in_dtype"], v["N"], v["U"], v["mean"], v["std"], v["use"], v["root"],
                                  v["cams"], v["C"], v["cam_of_row"], v["out"], None)
        msg = lib.p3d_last_error().decode()
        assert rc == E and msg.startswith("p3d_sample_world: ") and word in msg, (kw, rc, msg)

    for name in ("yn", "mean", "std", "use", "cams", "out"):
        call("null argument", **{name: None})
    for n in (0, -1, (1 << 20) + 1):
        call("N must be in 1 .. 2^20", N=n)
    for u in (0, -3, 97):
        call("U must be in 1 .. 96", U=u)
    for c in (0, -1, 65):
        call("C must be in 1 .. 64", C=c)
    for dt in (BF16, 7, -1):
        call("in_dtype F32 or F64", in_dtype=dt)
    call("out must be 16-byte aligned", out=p(20480 + 8))
    call("root must be 8-byte aligned", root=p(24576 + 4))
    assert F64 != F32


def test_key3d_mapping_plain_sh_and_world():
    from top_vae_3d_pose import data_handler
    cases = [
        # (key2d, camera_frame, key3d)
        ((9, "Walking", "Walking 1.54138969.h5"), True, (9, "Walking", "Walking 1.54138969.h5")),
        ((9, "Walking", "Walking 1.54138969.h5"), False, (9, "Walking", "Walking 1.h5")),
        ((11, "Sitting", "Sitting.60457274.h5-sh"), True, (11, "Sitting", "Sitting.60457274.h5")),
        ((11, "Sitting", "Sitting.60457274.h5-sh"), False, (11, "Sitting", "Sitting.h5")),
    ]
    for key2d, cf, key3d in cases:
        assert data_handler.get_key3d(key2d, camera_frame=cf) == key3d
        assert so.key3d_of(key2d, cf) == key3d


def test_camera_lookup_by_name():
    import predict_3dpose
    rcams, _, names = synth_cameras(np.random.default_rng(3))
    for subj in (9, 11):
        for ci, cname in enumerate(names[0]):
            key3d = (subj, "Walking", "Walking 1.%s.h5" % cname)
            idx, cam = predict_3dpose.sample_camera(rcams, key3d)
            assert idx == ci and cam is rcams[(subj, ci + 1)] and cam[-1] == cname
            assert so.the_camera(rcams, key3d) is cam
    with pytest.raises(ValueError, match="no camera named"):
        predict_3dpose.sample_camera(rcams, (9, "Walking", "Walking 1.00000000.h5"))
    # the cameras of the subject, not another's: a shuffled name order for subject 11
    rc2 = dict(rcams)
    rc2[(11, 1)], rc2[(11, 3)] = rcams[(11, 3)], rcams[(11, 1)]
    idx, cam = predict_3dpose.sample_camera(rc2, (11, "Walking", "Walking.%s.h5" % names[0][0]))
    assert idx == 2 and cam is rcams[(11, 1)]


@pytest.mark.parametrize("n_last", [1, 2, 7, 15, 16, 17, 300])
def test_picked_rows_are_the_references(n_last):
    import predict_3dpose
    np.random.seed(1234 + n_last)
    want = so.picked_rows(n_last)
    np.random.seed(1234 + n_last)
    got = predict_3dpose.pick_rows(n_last)
    np.testing.assert_array_equal(got, want)
    assert len(got) == min(15, n_last - 1)
    np.random.seed(1234 + n_last)
    perm = np.random.permutation(n_last)
    np.testing.assert_array_equal(got, perm[1:16])      # entry 0 of the permutation is never shown


def test_sample_dir_flag():
    import predict_3dpose
    p = predict_3dpose.build_parser()
    assert "--sample_dir" in p.format_help()
    assert p.parse_args([]).sample_dir == ""
    f = p.parse_args(["--sample", "--sample_dir", "out"])
    assert f.sample and f.sample_dir == "out"
    # not part of the hyper-parameter-encoded directory
    assert predict_3dpose.train_dir_for(f) == predict_3dpose.train_dir_for(p.parse_args([]))


def test_synthetic_with_camera_frame_is_refused():
    import predict_3dpose
    f = predict_3dpose.build_parser().parse_args(["--sample", "--synthetic", "--camera_frame"])
    with pytest.raises(ValueError, match="synthetic"):
        predict_3dpose.sample(f)
