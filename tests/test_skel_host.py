"""Host half of the rigid skeleton (include/p3d.h: p3d_skel_*; the drivers' --export_bvh flags): the
argument errors that answer before the GPU is touched, and the workspace sizes."""
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
    wb = int(lib.p3d_skel_workspace(N, S))

    def lengths(word, off=off, S=S, N=N, poses=p(), src=p(256), offd=p(512), L=p(768), used=p(1024), w=p(2048), wb=wb,
                host=True):
        oh = ctypes.c_void_p(off.ctypes.data) if host else None
        rc = lib.p3d_skel_lengths(poses, src, oh, offd, S, N, L, used, w, wb, None)
        msg = lib.p3d_last_error().decode()
        assert rc == E and msg.startswith("p3d_skel_lengths: ") and word in msg, (word, rc, msg)

    def pose(word, off=off, S=S, N=N, poses=p(), src=p(256), offd=p(512), L=p(768), outs=(p(1024), None, None, None),
             host=True, **_):
        oh = ctypes.c_void_p(off.ctypes.data) if host else None
        rc = lib.p3d_skel_pose(poses, src, oh, offd, S, N, L, *outs, None)
        msg = lib.p3d_last_error().decode()
        assert rc == E and msg.startswith("p3d_skel_pose: ") and word in msg, (word, rc, msg)

    I = lambda *v: np.array(v, np.int64)   # noqa: E731,E741
    for call in (lengths, pose):
        call("null", poses=None)
        call("null", L=None)
        call("null", host=False)
        call("null", offd=None)
        call("N must be", N=0)
        call("N must be", N=(1 << 20) + 1)
        call("S must be", S=0)
        call("S must be", S=N + 1, off=np.arange(N + 2, dtype=np.int64))
        call("start at 0", off=I(1, 9, 10, 30))
        call("end at N", off=I(0, 9, 10, 29))
        call("end at N", off=I(0, 9, 40, 30))
        call("decrease", off=I(0, 20, 10, 30))
        call("empty", off=I(0, 10, 10, 30))
    lengths("null", used=None)
    lengths("workspace", w=None)
    lengths("misaligned", w=p(2048 + 4))
    lengths("workspace too small", wb=wb - 1)
    pose("null outputs", outs=(None, None, None, None))
    del buf


def test_workspace_and_chunk():
    lib, _ = _lib()
    ws = lib.p3d_skel_workspace
    C = int(lib.p3d_skel_chunk())
    assert C >= 64
    assert ws(0, 1) == 0 and ws(10, 0) == 0 and ws(10, 11) == 0
    sizes = [1, 2, 9, C - 1, C, C + 1, 3 * C + 5, 1000, 4096, 1 << 20]
    for n in sizes:                                                       # non-decreasing in S (S <= N)
        prev = 0
        for s in sorted({min(n, v) for v in (1, 2, 3, 17, 240, 1000, n)}):
            assert ws(n, s) > 0 and ws(n, s) % 8 == 0 and ws(n, s) >= prev, (n, s)
            prev = ws(n, s)
    for s in (1, 2, 9):                                                   # non-decreasing in N
        col = [ws(n, s) for n in sizes if n >= s]
        assert col == sorted(col)
    # every chunk total S clips of N frames can have fits: S - 1 one-frame clips and the rest in one
    n, s = 10 * C + 7, 6
    most = (s - 1) + -(-(n - (s - 1)) // C)
    assert ws(n, s) >= (s + 1) * 4 + most * (16 * 8 + 8)


def test_driver_flags():
    import openpose_3dpose_sandbox as sandbox
    import openpose_3dpose_sandbox_realtime as realtime
    import predict_3dpose
    for mod in (predict_3dpose, sandbox, realtime):
        f = mod.build_parser().parse_args([])
        assert f.export_bvh is False and f.bvh_fps == 30.0
        f = mod.build_parser().parse_args(["--export_bvh", "--bvh_fps", "24"])
        assert f.export_bvh is True and f.bvh_fps == 24.0
    for mod in (sandbox, realtime):                                       # the 14-joint models have no skeleton
        with pytest.raises(SystemExit, match="17-joint model"):
            mod.main(["--verbose", "0", "--export_bvh", "--predict_14"])
