"""Host half of the live calls (include/p3d.h: p3d_live_reset / p3d_live_prepare / p3d_live_finish /
p3d_live_push): the argument errors that answer before the GPU is touched, and the state and
workspace sizes."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "3d-pose-baseline_amd", "libp3d.so")


def _lib():
    if not os.path.exists(LIB):
        pytest.skip("libp3d.so not built")
    import _p3d
    return _p3d.lib(), _p3d.P3D_ERR_ARG


def _fake():
    """A 256-byte aligned address inside a live host buffer: stands for every device pointer of a
    call that must answer before anything is launched."""
    buf = (ctypes.c_double * 8192)()
    a = ctypes.addressof(buf)
    return buf, a + (-a) % 256


I64 = lambda *v: np.array(v, np.int64)   # noqa: E731
I32 = lambda *v: np.array(v, np.int32)   # noqa: E731
S, N = 3, 6
OFF, FRAME, KIND = I64(0, 5, 5, 6), I32(0, 1, 2, 3, 4, 9), I32(1, 1, 1, 1, 2, 2)
PUSH = I32(8, -1, 13)


def test_prepare_and_finish_argument_errors_without_a_gpu():
    lib, E = _lib()
    buf, a = _fake()
    p = lambda off=0: ctypes.c_void_p(a + off)   # noqa: E731
    h = lambda arr: None if arr is None else ctypes.c_void_p(arr.ctypes.data)   # noqa: E731

    def prep(word, off=OFF, frame=FRAME, kind=KIND, push=PUSH, S=S, N=N, smooth=1, xy=p(), U2=32, state=p(256), x=p(512),
             xy_s=p(768), m2=p()):
        rc = lib.p3d_live_prepare(xy, h(push), h(off), h(frame), h(kind), S, N, smooth, m2, p(), p(), U2, state, x, xy_s,
                                  None)
        msg = lib.p3d_last_error().decode()
        assert rc == E and msg.startswith("p3d_live_prepare: ") and word in msg, (word, rc, msg)

    def fin(word, off=OFF, frame=FRAME, S=S, N=N, y=p(), xy_s=p(256), U3=48, D3=96, state=p(512), poses=p(768), m3=p(),
            **_):
        rc = lib.p3d_live_finish(y, h(off), h(frame), S, N, xy_s, m3, p(), p(), U3, D3, 1, state, poses, None, None)
        msg = lib.p3d_last_error().decode()
        assert rc == E and msg.startswith("p3d_live_finish: ") and word in msg, (word, rc, msg)

    for call in (prep, fin):
        call("null row_off", off=None)
        call("null row_frame", frame=None)
        call("S must be", S=0)
        call("S must be", S=(1 << 16) + 1)
        call("N must be", N=-1)
        call("N must be", N=5 * S + 1)
        call("start at 0", off=I64(1, 5, 5, 6))
        call("end at N", off=I64(0, 5, 5, 5))
        call("end at N", off=I64(0, 5, 7, 6))
        call("decrease", off=I64(0, 5, 4, 6))
        call("more than 5 rows", off=I64(0, 6, 6, 6))
        call("row_frame must be", frame=I32(0, 1, 2, -3, 4, 9))
        call("state", state=None)
        call("state", state=p(256 + 4))
    prep("null statistics", m2=None)
    prep("null xy_in", xy=None)
    prep("null xy_in or push_frame", push=None)
    prep("null row_kind", kind=None)
    prep("row_kind must be in 0..3", kind=I32(1, 1, 1, 1, 2, 4))
    prep("row_kind must be in 0..3", kind=I32(1, 1, -1, 1, 2, 2))
    prep("without smoothing", smooth=0)
    prep("U2", U2=65)
    prep("U2", U2=0)
    prep("null x or xy_s", x=None)
    prep("null x or xy_s", xy_s=None)
    fin("null statistics", m3=None)
    fin("null y", y=None)
    fin("null y", poses=None)
    fin("96", D3=48)
    fin("U3", U3=97)
    del buf


def test_push_and_reset_argument_errors_without_a_model():
    lib, E = _lib()
    buf, a = _fake()
    p = lambda off=0: ctypes.c_void_p(a + off)   # noqa: E731
    h = lambda arr: None if arr is None else ctypes.c_void_p(arr.ctypes.data)   # noqa: E731
    wb = int(lib.p3d_live_push_workspace(S, 32, 48, 0))

    def push(word, K=0, row0=0, off=OFF, frame=FRAME, kind=KIND, push=PUSH, S=S, N=N, smooth=1, xy=p(), U2=32, U3=48,
             D3=96, state=p(256), xy_s=p(512), poses=p(768), var=None, fst=None, w=p(1024), wb=wb, m2=p()):
        rc = lib.p3d_live_push(None, None, K, 0, row0, state, fst, None, xy, h(push), h(off), h(frame), h(kind), S, N, m2,
                               p(), p(), U2, p(), p(), p(), U3, D3, 1, smooth, xy_s, poses, None, var, w, wb, None)
        msg = lib.p3d_last_error().decode()
        assert rc == E and msg.startswith("p3d_live_push: ") and word in msg, (word, rc, msg)

    push("null model")                                   # everything else is in order: the model is asked for last
    push("null statistics", m2=None)
    push("null xy_s or poses", xy_s=None)
    push("null xy_s or poses", poses=None)
    push("null xy_in", xy=None)
    push("null xy_in or push_frame", push=None)
    push("null row_off", off=None)
    push("null row_frame", frame=None)
    push("null row_kind", kind=None)
    push("S must be", S=0)
    push("N must be", N=5 * S + 1)
    push("N must be", N=-1)
    push("start at 0", off=I64(2, 5, 5, 6))
    push("end at N", off=I64(0, 5, 5, 7))
    push("decrease", off=I64(0, 5, 4, 6))
    push("more than 5 rows", off=I64(0, 0, 6, 6))
    push("row_frame must be", frame=I32(-1, 1, 2, 3, 4, 9))
    push("row_kind must be in 0..3", kind=I32(1, 1, 1, 1, 2, 7))
    push("without smoothing", smooth=0)
    push("state", state=None)
    push("state", state=p(256 + 2))
    push("U2", U2=65)
    push("U3", U3=97)
    push("96", D3=95)
    for K in (-1, 65):
        push("K must be", K=K)
    push("eps_row0", row0=-1)
    push("workspace", w=None)
    push("256-byte aligned", w=p(1024 + 8))
    push("workspace too small", wb=wb - 1)
    push("need a filter", K=2)
    push("need a filter", var=p(2048))
    push("need a filter", fst=p(2048))
    for args, word in (((None, S, -1), b"state"), ((p(4), S, -1), b"state"), ((p(), 0, -1), b"S must be"),
                       ((p(), S, S), b"slot must be")):
        assert lib.p3d_live_reset(*args, None) == E and word in lib.p3d_last_error(), args
        assert lib.p3d_last_error().startswith(b"p3d_live_reset: ")
    del buf


def test_state_and_workspace_sizes():
    lib, _ = _lib()
    sb, ws = lib.p3d_live_state_bytes, lib.p3d_live_push_workspace
    assert sb(0, 48) == 0 and sb(1, 0) == 0 and sb(1, 97) == 0 and sb((1 << 16) + 1, 48) == 0
    assert ws(0, 32, 48, 0) == 0 and ws(1, 0, 48, 0) == 0 and ws(1, 32, 0, 1) == 0
    prev = 0
    for s in (1, 2, 3, 4, 5, 64, 1000, 1 << 16):
        # ring [16, 36] | last [36] | good [96] float64 and the good frame int32, per slot
        assert sb(s, 48) % 256 == 0 and sb(s, 48) >= s * ((17 * 36 + 96) * 8 + 4) and sb(s, 48) > prev
        prev = sb(s, 48)
        assert ws(s, 32, 48, 0) % 256 == 0 and ws(s, 32, 48, 0) >= 5 * s * (32 + 48) * 4
        assert ws(s, 32, 48, 1) >= ws(s, 32, 48, 0) + 5 * s * 48 * 4
