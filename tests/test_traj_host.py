"""Host half of the root trajectory (include/p3d.h: p3d_root_trajectory; the drivers'
--root_trajectory flags): the argument errors that answer before the GPU is touched, and the
workspace sizes."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
LIB = os.path.join(ROOT, "3d-pose-baseline_amd", "libp3d.so")


def _lib():
    if not os.path.exists(LIB):
        pytest.skip("libp3d.so not built")
    import _p3d
    return _p3d.lib(), _p3d.P3D_ERR_ARG


def test_argument_errors_without_a_gpu():
    lib, E = _lib()
    buf = (ctypes.c_double * 8192)()                      # stands for every device pointer: nothing is launched
    a = ctypes.addressof(buf)
    a += (-a) % 256
    p = lambda off=0: ctypes.c_void_p(a + off)   # noqa: E731
    N, S = 30, 3
    off = np.array([0, 9, 10, 30], np.int64)
    wb = int(lib.p3d_root_trajectory_workspace(N, 4))
    assert wb > 0

    def call(word, off=off, S=S, N=N, poses=p(), xy=p(256), src=p(512), offd=p(768), focal=1145.0, cx=512.0, cy=515.0, h=4,
             outs=(p(1024), p(1280), p(1536), p(1792)), w=p(2048), wb=wb, host=True):
        oh = ctypes.c_void_p(off.ctypes.data) if host else None
        rc = lib.p3d_root_trajectory(poses, xy, src, oh, offd, S, N, focal, cx, cy, h, *outs, w, wb, None)
        msg = lib.p3d_last_error().decode()
        assert rc == E and msg.startswith("p3d_root_trajectory: ") and word in msg, (word, rc, msg)

    I = lambda *v: np.array(v, np.int64)   # noqa: E731,E741
    call("null", poses=None)
    call("null", xy=None)
    call("null", host=False)
    call("null", offd=None)
    call("null outputs", outs=(None, None, None, None))
    call("N must be", N=0)
    call("N must be", N=(1 << 20) + 1)
    call("S must be", S=0)
    call("S must be", S=N + 1, off=np.arange(N + 2, dtype=np.int64))
    call("start at 0", off=I(1, 9, 10, 30))
    call("end at N", off=I(0, 9, 10, 29))
    call("end at N", off=I(0, 9, 40, 30))
    call("decrease", off=I(0, 20, 10, 30))
    call("empty", off=I(0, 10, 10, 30))
    for bad in (0.0, -1145.0, float("inf"), float("nan")):
        call("focal", focal=bad)
    for bad in (float("inf"), float("-inf"), float("nan")):
        call("principal point", cx=bad)
        call("principal point", cy=bad)
    call("smooth_half", h=-1)
    call("smooth_half", h=33)
    call("workspace", w=None)
    call("misaligned", w=p(2048 + 4))
    call("workspace too small", wb=wb - 1)
    call("workspace too small", h=32, wb=int(lib.p3d_root_trajectory_workspace(N, 32)) - 1)
    del buf


def test_workspace_and_rows():
    lib, _ = _lib()
    ws = lib.p3d_root_trajectory_workspace
    W = int(lib.p3d_root_trajectory_rows())
    assert 1 <= W <= 256
    assert ws(0, 4) == 0 and ws(-1, 4) == 0 and ws((1 << 20) + 1, 4) == 0 and ws(10, -1) == 0 and ws(10, 33) == 0
    sizes = [1, 2, 9, W - 1, W, W + 1, 3 * W + 5, 1000, 4096, 1 << 20]
    for h in (1, 4, 32):
        col = [ws(n, h) for n in sizes if n >= 1]
        assert col == sorted(col) and all(c > 0 and c % 8 == 0 for c in col)      # monotone in N
        for n in sizes:
            assert ws(n, h) >= n * (3 * 8 + 4)                                    # the raw rows and the flags fit
    for n in sizes:                                                               # no window: nothing to hold
        assert ws(n, 0) == 0


def test_driver_flags():
    import openpose_3dpose_sandbox as sandbox
    import openpose_3dpose_sandbox_realtime as realtime
    import predict_3dpose
    for mod in (predict_3dpose, sandbox, realtime):
        f = mod.build_parser().parse_args([])
        assert f.root_trajectory is False and f.focal is None and f.principal is None and f.trajectory_smooth == 4
        f = mod.build_parser().parse_args(["--root_trajectory", "--focal", "1145", "--principal", "512", "515",
                                           "--trajectory_smooth", "0"])
        assert f.root_trajectory is True and f.focal == 1145.0 and f.principal == [512.0, 515.0] and f.trajectory_smooth == 0
    for mod in (sandbox, realtime):                                       # the camera has no silent default
        with pytest.raises(SystemExit, match="1145"):
            mod.main(["--verbose", "0", "--root_trajectory"])
        with pytest.raises(SystemExit, match=r"\(512, 515\)"):
            mod.main(["--verbose", "0", "--root_trajectory", "--focal", "1000"])
        with pytest.raises(SystemExit, match="trajectory_smooth"):
            mod.main(["--verbose", "0", "--root_trajectory", "--focal", "1000", "--principal", "1", "2",
                      "--trajectory_smooth", "33"])


def test_python_checks_need_no_gpu():
    import openpose_frontend as of
    for bad in (dict(focal=0.0), dict(focal=float("nan")), dict(center=(1.0, float("inf"))), dict(center=(1.0,)),
                dict(smooth_half=33), dict(smooth_half=-1), dict(smooth_half=1.5)):
        kw = dict(dict(focal=1145.0, center=(512.0, 515.0), smooth_half=4), **bad)
        with pytest.raises(ValueError):
            of._check_camera(kw["focal"], kw["center"], kw["smooth_half"])
    assert of._check_camera(1145, [512, 515], 4) == (1145.0, 512.0, 515.0, 4)
    with pytest.raises(ValueError, match="traj"):
        of.export_trajectory("/nonexistent", [0, 1], dict(traj=np.zeros((3, 3)), resid=np.zeros(2), valid=np.ones(2), camera={}))


def test_export_trajectory(tmp_path):
    import json
    import openpose_frontend as of
    r = dict(traj=np.array([[1.0, 2.0, 3000.0], [0.0, 0.0, 0.0]]), resid=np.array([0.5, 0.0]), valid=np.array([True, False]),
             camera=dict(focal=1145.0, center=[512.0, 515.0], smooth_half=4))
    path = of.export_trajectory(str(tmp_path / "out"), [7, 8], r)
    assert path == str(tmp_path / "out" / "trajectory.json")
    got = json.load(open(path))
    assert got == {"trajectory": {"7": [1.0, 2.0, 3000.0], "8": [0.0, 0.0, 0.0]}, "resid": [0.5, 0.0],
                   "valid": [True, False], "camera": {"focal": 1145.0, "center": [512.0, 515.0], "smooth_half": 4}}
