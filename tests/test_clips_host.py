"""Host half of the batched clip call (include/p3d.h: p3d_clips_*; openpose_frontend.read_clips /
check_clips / export_maya_clips; the driver's flags): the argument errors that answer before the
GPU is touched, the workspace sizes, the directory reader and the per-clip export."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
LIB = os.path.join(ROOT, "3d-pose-baseline_amd", "libp3d.so")

import openpose_frontend as of  # noqa: E402

GOLD = os.path.join(HERE, "golden", "clip_goldens.npz")


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


def test_prepare_and_finish_argument_errors_without_a_gpu():
    lib, E = _lib()
    buf, a = _fake()
    p = lambda off=0: ctypes.c_void_p(a + off)   # noqa: E731
    N, S = 30, 3
    off = np.array([0, 9, 10, 30], np.int64)
    wb = int(lib.p3d_clips_workspace(N, S))

    def prep(word, off=off, S=S, N=N, smooth=1, xy=p(), offd=p(256), x=p(512), xy_s=p(768), w=p(1024), wb=wb, U2=32,
             host=True):
        oh = ctypes.c_void_p(off.ctypes.data) if host else None
        rc = lib.p3d_clips_prepare(xy, oh, offd, S, N, smooth, p(), p(), p(), U2, x, xy_s, w, wb, None)
        msg = lib.p3d_last_error().decode()
        assert rc == E and msg.startswith("p3d_clips_prepare: ") and word in msg, (word, rc, msg)

    def fin(word, off=off, S=S, N=N, y=p(), offd=p(256), poses=p(512), w=p(1024), wb=wb, D3=96, U3=48, host=True):
        oh = ctypes.c_void_p(off.ctypes.data) if host else None
        rc = lib.p3d_clips_finish(y, oh, offd, S, N, p(), p(), p(), p(), U3, D3, 1, poses, None, w, wb, None)
        msg = lib.p3d_last_error().decode()
        assert rc == E and msg.startswith("p3d_clips_finish: ") and word in msg, (word, rc, msg)

    I = lambda *v: np.array(v, np.int64)   # noqa: E731,E741
    for call in (prep, fin):
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
        call("workspace", w=None)
        call("workspace", w=p(1024 + 4))
        call("workspace too small", wb=wb - 1)
    prep("null argument", xy=None)
    prep("null argument", x=None)
    prep("alias", xy_s=p())
    prep("U2", U2=65)
    for n in range(2, 9):                                   # a clip of 2..8 frames with smoothing on
        prep("min 9 frames", off=I(0, 9, 9 + n, 30))
        prep("min 9 frames", off=I(0, n, 20, 30))
    fin("null argument", y=None)
    fin("null argument", poses=None)
    fin("96", D3=48)
    fin("U3", U3=97)
    del buf


def test_lift_argument_errors_without_a_model():
    lib, E = _lib()
    buf, a = _fake()
    p = lambda off=0: ctypes.c_void_p(a + off)   # noqa: E731
    off = np.array([0, 9, 30], np.int64)
    rc = lib.p3d_clips_lift(None, None, 0, None, 0, 0, p(), ctypes.c_void_p(off.ctypes.data), p(256), 2, 30, 1, p(), p(),
                            p(), 32, p(), p(), p(), 48, 96, 1, p(512), p(768), None, None, None, None, p(1024), 1 << 20,
                            None)
    assert rc == E and b"p3d_clips_lift: null model" in lib.p3d_last_error()
    del buf


def test_workspace_sizes():
    lib, _ = _lib()
    ws, lws = lib.p3d_clips_workspace, lib.p3d_clips_lift_workspace
    C = int(lib.p3d_clip_chunk())
    assert ws(0, 1) == 0 and ws(10, 0) == 0 and ws(10, 11) == 0 and lws(10, 1, 0, 48, 0) == 0
    sizes = [1, 2, 9, C - 1, C, C + 1, 3 * C + 5, 1000, 4096, 1 << 20]
    for n in sizes:
        assert ws(n, 1) >= lib.p3d_clip_workspace(n)                      # S = 1: at least the single clip's
        assert lws(n, 1, 32, 48, 0) >= lib.p3d_clip_lift_workspace(n, 32, 48)
        assert lws(n, 1, 32, 48, 1) >= lws(n, 1, 32, 48, 0) + n * 48 * 4
        prev = 0
        for s in sorted({min(n, v) for v in (1, 2, 3, 17, 1000, n)}):     # non-decreasing in S (S <= N)
            assert ws(n, s) % 256 == 0 and lws(n, s, 32, 48, 0) % 256 == 0 and lws(n, s, 32, 48, 1) % 256 == 0
            assert ws(n, s) >= prev and ws(n, s) > 0
            prev = ws(n, s)
    for s in (1, 2, 9):                                                   # non-decreasing in N
        col = [ws(n, s) for n in sizes if n >= s]
        assert col == sorted(col)
        col = [lws(n, s, 32, 48, 1) for n in sizes if n >= s]
        assert col == sorted(col)
    # every chunk total S clips of N frames can have fits: S - 1 one-frame clips and the rest in one
    n, s = 10 * C + 7, 6
    most = (s - 1) + -(-(n - (s - 1)) // C)
    assert ws(n, s) >= 256 + most * (8 + 36 * 12)


def write_clip(d, raw, start=0):
    os.makedirs(d, exist_ok=True)
    for i, row in enumerate(raw):
        with open(os.path.join(d, "clip_%012d_keypoints.json" % (start + i)), "w") as f:
            json.dump({"people": [{"pose_keypoints_2d": [float(v) for v in row]}]}, f)


def test_read_clips_and_check_clips(tmp_path):
    with np.load(GOLD, allow_pickle=False) as z:
        raw = {n: z["raw_coco_%d" % n] for n in (9, 10, 23)}
        xy = {n: z["xy_coco_%d" % n] for n in (9, 10, 23)}
    root = tmp_path / "clips"
    write_clip(str(root / "b_second"), raw[10], start=5)
    write_clip(str(root / "a_first"), raw[23])
    write_clip(str(root / "c_third"), raw[9])
    (root / "empty_dir").mkdir()                                          # no frame files: not a clip
    (root / "notes.json").write_text("{}")                                # a plain file: ignored
    names, numbers, clips = of.read_clips(str(root))
    assert names == ["a_first", "b_second", "c_third"]
    assert [len(c) for c in clips] == [23, 10, 9]
    np.testing.assert_array_equal(numbers[1], np.arange(5, 15))
    for c, n in zip(clips, (23, 10, 9)):
        assert c.dtype == np.float64 and c.tobytes() == xy[n].tobytes()
    of.check_clips(numbers, True, names)
    write_clip(str(root / "d_short"), raw[9][:5])
    names, numbers, clips = of.read_clips(str(root))
    with pytest.raises(ValueError, match="d_short.*min 9 frames"):
        of.check_clips(numbers, True, names)
    of.check_clips(numbers, False, names)
    with pytest.raises(ValueError, match="no clip directories"):
        of.read_clips(str(root / "empty_dir"))


def test_export_per_clip(tmp_path):
    rng = np.random.default_rng(4)
    res, nums = [], [np.arange(3, 7), np.arange(2)]
    for n in (4, 2):
        res.append({"poses": rng.uniform(-900, 900, (n, 96)), "xy_s": rng.uniform(0, 900, (n, 36)),
                    "poses_unfiltered": rng.uniform(-900, 900, (n, 96))})
    paths = of.export_maya_clips(str(tmp_path / "out"), ["one", "two"], nums, res, unfiltered=True)
    assert [os.path.relpath(q, str(tmp_path / "out")) for q in paths[1]] == [
        os.path.join("two", f) for f in ("3d_data.json", "2d_data.json", "3d_data_unfiltered.json")]
    for r, fn, ps in zip(res, nums, paths):
        three, two, unf = (json.load(open(q)) for q in ps)
        assert sorted(three, key=int) == sorted(unf, key=int) == sorted(two, key=int) == [str(f) for f in fn]
        for i, f in enumerate(fn):
            got = np.array([three[str(f)][str(j)]["translate"] for j in range(32)]).reshape(96)
            gotu = np.array([unf[str(f)][str(j)]["translate"] for j in range(32)]).reshape(96)
            assert got.tobytes() == r["poses"][i].tobytes() and gotu.tobytes() == r["poses_unfiltered"][i].tobytes()
    plain = of.export_maya_clips(str(tmp_path / "plain"), ["one", "two"], nums, res)
    assert all(len(q) == 2 for q in plain) and not os.path.exists(str(tmp_path / "plain" / "one" / "3d_data_unfiltered.json"))
    with pytest.raises(ValueError):
        of.export_maya_clips(str(tmp_path / "bad"), ["one"], nums, res)


def test_driver_flags():
    import openpose_3dpose_sandbox as sandbox
    f = sandbox.build_parser().parse_args([])
    assert f.clips_root is None and f.vae_filter is None and f.filter_samples is None and not f.export_unfiltered
    assert (f.latent_dim, f.enc_dim, f.dec_dim) == (24, [40, 32], [32, 40])      # args_def's defaults
    f = sandbox.build_parser().parse_args(["--clips_root", "d", "--vae_filter", "w.npz", "--filter_samples", "4",
                                           "--export_unfiltered", "--enc_dim", "48", "24"])
    assert (f.clips_root, f.vae_filter, f.filter_samples, f.export_unfiltered, f.enc_dim) == ("d", "w.npz", 4, True, [48, 24])
    for argv in (["--filter_samples", "2"], ["--export_unfiltered"]):            # both need a filter
        with pytest.raises(SystemExit, match="need --vae_filter"):
            sandbox.main(["--verbose", "0"] + argv)
