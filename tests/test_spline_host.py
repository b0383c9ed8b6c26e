"""Host half of the spline resampling (include/p3d.h: p3d_clips_resample*, p3d_clips_lift_resampled*;
the drivers' --spline_resample): the argument errors that answer before the GPU is touched, each
message starting with the call's name, and the workspace sizes."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "3d-pose-baseline_amd"))
LIB = os.path.join(ROOT, "3d-pose-baseline_amd", "libp3d.so")


def _lib():
    if not os.path.exists(LIB):
        pytest.skip("libp3d.so not built")
    import _p3d
    return _p3d.lib(), _p3d.P3D_ERR_ARG


def test_resample_argument_errors_without_a_gpu():
    lib, E = _lib()
    buf = (ctypes.c_double * 8192)()                      # stands for every device pointer: nothing is launched
    a = ctypes.addressof(buf)
    a += (-a) % 256
    p = lambda off=0: ctypes.c_void_p(a + off)   # noqa: E731
    N, S = 30, 3
    off = np.array([0, 9, 13, 30], np.int64)
    wb = int(lib.p3d_clips_resample_workspace(N, S, 2))
    assert wb > 0

    def call(word, off=off, S=S, N=N, R=2, xy_s=p(), offd=p(256), m2=p(512), s2=p(768), u2=p(1024), U2=32, x=p(1280),
             xy_r=p(1536), off_out=p(1792), info=p(2048), w=p(4096), wb=wb, host=True):
        oh = ctypes.c_void_p(off.ctypes.data) if host else None
        rc = lib.p3d_clips_resample(xy_s, oh, offd, S, N, R, m2, s2, u2, U2, x, xy_r, off_out, info, w, wb, None)
        msg = lib.p3d_last_error().decode()
        assert rc == E and msg.startswith("p3d_clips_resample: ") and word in msg, (word, rc, msg)

    I = lambda *v: np.array(v, np.int64)   # noqa: E731,E741
    for k in ("xy_s", "m2", "s2", "u2", "x", "xy_r", "off_out"):
        call("null argument", **{k: None})
    call("null clip offsets", host=False)
    call("null clip offsets", offd=None)
    call("N must be", N=0)
    call("N must be", N=(1 << 20) + 1)
    call("S must be", S=0)
    call("S must be", S=N + 1, off=np.arange(N + 2, dtype=np.int64))
    call("start at 0", off=I(1, 9, 13, 30))
    call("end at N", off=I(0, 9, 13, 29))
    call("end at N", off=I(0, 9, 40, 30))
    call("decrease", off=I(0, 20, 10, 30))
    call("empty", off=I(0, 10, 10, 30))
    call("R must be in 1..16", R=0)
    call("R must be in 1..16", R=17)
    call("R must be in 1..16", R=-3)
    call("clip 1: need more frames, min 4 frames", off=I(0, 9, 12, 30))
    call("clip 0: need more frames, min 4 frames", off=I(0, 1, 13, 30))
    call("clip 0: at most 65536 frames", S=1, N=65537, off=I(0, 65537), R=1)
    call("R * N must be at most 1048576", S=1, N=(1 << 16) + 1, off=I(0, (1 << 16) + 1), R=16)
    call("R * N must be at most 1048576", S=2, N=1 << 17, off=I(0, 1 << 16, 1 << 17), R=9)
    call("U2 must be", U2=0)
    call("U2 must be", U2=65)
    call("alias", xy_r=p())
    call("null or misaligned workspace", w=None)
    call("null or misaligned workspace", w=p(4096 + 4))
    call("workspace too small", wb=wb - 1)
    del buf


def test_lift_resampled_refuses_before_the_model_is_read():
    lib, E = _lib()
    rc = lib.p3d_clips_lift_resampled(None, None, 0, None, 0, 0, None, None, None, 1, 9, 1, None, None, None, 32,
                                      None, None, None, 48, 96, 1, None, None, None, None, None, None, 2, None, None,
                                      None, None, 0, None)
    msg = lib.p3d_last_error().decode()
    assert rc == E and msg == "p3d_clips_lift_resampled: null model", msg


def test_workspace_sizes():
    lib, _ = _lib()
    ws, lws = lib.p3d_clips_resample_workspace, lib.p3d_clips_lift_resampled_workspace
    assert ws(0, 1, 2) == 0 and ws(10, 0, 2) == 0 and ws(10, 11, 2) == 0 and ws(10, 1, 0) == 0 and ws(10, 1, 17) == 0
    assert lws(10, 1, 0, 32, 48, 0) == 0 and lws(10, 1, 17, 32, 48, 0) == 0 and lws(10, 1, 2, 0, 48, 0) == 0
    a256 = lambda b: (b + 255) // 256 * 256   # noqa: E731
    for n, s in ((4, 1), (9, 1), (30, 3), (300, 1), (442, 4), (72000, 240), (1 << 16, 1)):
        coef = 36 * (n + 4 * s)                               # every curve's m + 4 knots / coefficients
        want = 2 * a256(coef * 8) + a256(s * 36 * 5 * 4) + a256(coef * 24 * 8)
        for r in (1, 2, 10, 16):
            assert ws(n, s, r) == want, (n, s, r)
            head = lib.p3d_clips_workspace(n, s) + want + lib.p3d_clips_workspace(r * n, s)
            for filt in (0, 1):
                rows = a256(r * n * 32 * 4) + (1 + filt) * a256(r * n * 48 * 4)
                assert lws(n, s, r, 32, 48, filt) == head + rows, (n, s, r, filt)
    col = [ws(n, 1, 2) for n in (4, 9, 64, 300, 4096)]
    assert col == sorted(col) and len(set(col)) == len(col)


def test_driver_flags(monkeypatch):
    import openpose_3dpose_sandbox as sandbox
    import openpose_3dpose_sandbox_realtime as realtime
    import predict_3dpose
    monkeypatch.setattr(predict_3dpose, "FLAGS", predict_3dpose.FLAGS)       # (main() replaces it: put back afterwards)
    for mod in (sandbox, realtime):
        assert mod.build_parser().parse_args([]).spline_resample is None
        assert mod.build_parser().parse_args(["--spline_resample", "10"]).spline_resample == 10
    for bad in ("0", "17"):
        with pytest.raises(SystemExit, match="1..16"):
            sandbox.main(["--verbose", "0", "--spline_resample", bad])
    with pytest.raises(SystemExit, match="--spline_resample R is its --multiplier 1/R"):
        sandbox.main(["--verbose", "0", "--interpolation"])
    for flags in (["--interpolation"], ["--spline_resample", "2"]):                 # a stream cannot be resampled
        with pytest.raises(SystemExit, match="not causal"):
            realtime.main(["--verbose", "0"] + flags)
