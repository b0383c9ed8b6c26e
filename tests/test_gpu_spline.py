"""The spline resampling on the GPU (include/p3d.h: p3d_clips_resample) against
tests/spline_oracle.py, which states the same float64 operations in the same order: the info records
and every knot equal, the coefficients and the resampled rows compared as bytes (no contraction, IEEE
division and square root on both sides), x as bytes against p3d_clips_prepare(xy_r, smooth = 0).

The clips are built from the tracks of tests/golden/spline_goldens.npz (the curves scipy was recorded
on, tests/test_spline_oracle.py), a clip's 36 columns cycling through the tracks of its length, so the
oracle fits a handful of distinct curves per clip."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-pose-baseline_amd"))
sys.path.insert(0, HERE)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import _p3d  # noqa: E402
import data_pipeline as dp  # noqa: E402
import data_utils  # noqa: E402
import spline_oracle as so  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "spline_goldens.npz"))
NAMES = [str(n) for n in GOLD["names"]]
USE2, _ = data_utils.dimension_sets(2)
GUARD, SENTINEL = 64, -7.0
WRONG = lambda N: ([0, 5, 3, N + 900, N], [-40, 1 << 40, -1, 7, 2], [N, N, N, N, N], [0, 0, 0, 0, 0],   # noqa: E731
                   [0, N, N, N, N])                          # test_gpu_skel.py's five tables (four clips)
_RNG = np.random.default_rng(31)
MEAN2, STD2 = _RNG.uniform(200, 600, 64), _RNG.uniform(50, 150, 64)

_FITS = {}


def track(name):
    return GOLD["y_%d" % NAMES.index(name)]


def oracle(y):
    """so.fit of one track, computed once per distinct track."""
    key = np.ascontiguousarray(y, np.float64).tobytes()
    if key not in _FITS:
        _FITS[key] = so.fit(y)
    return _FITS[key]


def clip_of(m, extra=()):
    """[m, 36]: the columns cycle through the golden tracks of m frames; `extra` tracks take the last columns."""
    cols = [track("%s_%d" % (k, m)) for k in ("move", "move2", "still", "jumpy", "zerorun")]
    xy = np.stack([cols[c % len(cols)] for c in range(36)], axis=1)
    for i, name in enumerate(extra):
        xy[:, 35 - i] = track(name)
    return np.ascontiguousarray(xy)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def run(xy_s, off, R, off_dev=None, with_info=True):
    """p3d_clips_resample on fresh buffers with guard words around every output and the workspace ->
    dict(x [R N, 32], xy_r [R N, 36], off_out [S + 1], info [S, 36, 5], t, c: the workspace's coefficient areas)."""
    lib, p = _p3d.lib(), _p3d.ptr
    off = np.ascontiguousarray(off, np.int64)
    S, N = len(off) - 1, int(off[-1])
    U2 = len(USE2)
    d_xy = torch.from_numpy(np.ascontiguousarray(xy_s, np.float64)).cuda()
    d_off = torch.from_numpy(off if off_dev is None else np.ascontiguousarray(off_dev, np.int64)).cuda()
    m2, s2, u2 = dp.as_device(MEAN2), dp.as_device(STD2), dp._dims(USE2, 64, "t")
    g = lambda n, dt: torch.full((n + 2 * GUARD,), SENTINEL, dtype=dt, device="cuda")   # noqa: E731
    nbytes = int(lib.p3d_clips_resample_workspace(N, S, R))
    assert nbytes % 256 == 0
    bufs = dict(x=g(R * N * U2, torch.float32), xy_r=g(R * N * 36, torch.float64), off_out=g(S + 1, torch.int64),
                info=g(S * 36 * 5, torch.int32), work=g(nbytes // 8, torch.float64))
    at = lambda k: p(bufs[k]) + GUARD * bufs[k].element_size()   # noqa: E731
    _p3d.check(lib.p3d_clips_resample(p(d_xy), off.ctypes.data, p(d_off), S, N, R, p(m2), p(s2), p(u2), U2, at("x"),
                                      at("xy_r"), at("off_out"), at("info") if with_info else None, at("work"), nbytes,
                                      _p3d.stream_handle()), "p3d_clips_resample")
    torch.cuda.synchronize()
    out = {}
    for k, t in bufs.items():
        h = t.cpu().numpy()
        assert (h[:GUARD] == SENTINEL).all() and (h[-GUARD:] == SENTINEL).all(), "%s: a guard word changed" % k
        out[k] = h[GUARD:-GUARD]
    a256 = lambda b: (b + 255) // 256 * 256   # noqa: E731
    coef = 36 * (N + 4 * S)
    cb = a256(coef * 8) // 8
    work = out.pop("work")
    out["t"], out["c"] = work[:coef], work[cb:cb + coef]
    if not with_info:
        assert (out["info"] == SENTINEL).all()
        out["info"] = work[2 * cb:2 * cb + a256(S * 36 * 5 * 4) // 8].view(np.int32)[:S * 36 * 5].copy()
    out["x"], out["xy_r"] = out["x"].reshape(R * N, U2), out["xy_r"].reshape(R * N, 36)
    out["info"] = out["info"].reshape(S, 36, 5)
    return out


def prepare_unsmoothed(xy_r, off_r):
    """x of p3d_clips_prepare(xy_r, smooth = 0) under the resampled offsets."""
    lib, p = _p3d.lib(), _p3d.ptr
    off_r = np.ascontiguousarray(off_r, np.int64)
    S, N = len(off_r) - 1, int(off_r[-1])
    d_xy, d_off = torch.from_numpy(np.ascontiguousarray(xy_r)).cuda(), torch.from_numpy(off_r).cuda()
    m2, s2, u2 = dp.as_device(MEAN2), dp.as_device(STD2), dp._dims(USE2, 64, "t")
    x = torch.empty((N, len(USE2)), dtype=torch.float32, device="cuda")
    xy_s = torch.empty((N, 36), dtype=torch.float64, device="cuda")
    nbytes = int(lib.p3d_clips_workspace(N, S))
    work = torch.empty((nbytes // 8 + 1,), dtype=torch.float64, device="cuda")
    _p3d.check(lib.p3d_clips_prepare(p(d_xy), off_r.ctypes.data, p(d_off), S, N, 0, p(m2), p(s2), p(u2), len(USE2), p(x),
                                     p(xy_s), p(work), nbytes, _p3d.stream_handle()), "p3d_clips_prepare")
    torch.cuda.synchronize()
    assert same(xy_s.cpu().numpy(), np.ascontiguousarray(xy_r))
    return x.cpu().numpy()


def check_clip(got, xy, lo, s, R, what):
    """Clip s (rows lo .. of the batch) of a result against the oracle, curve by curve."""
    m = xy.shape[0]
    at = np.arange(R * m, dtype=np.float64) * (1.0 / R)
    evals = {}
    for col in range(36):
        f = oracle(xy[:, col])
        w = "%s clip %d column %d" % (what, s, col)
        np.testing.assert_array_equal(got["info"][s, col], so.info_record(f), err_msg=w)
        base, n = 36 * (lo + 4 * s) + col * (m + 4), f["n"]
        np.testing.assert_array_equal(got["t"][base:base + n], f["t"], err_msg=w + " knots")
        key = xy[:, col].tobytes()
        if key not in evals:
            evals[key] = so.splev(f["t"], f["c"], at)
        if not np.isfinite(xy[:, col]).all():                 # (a NaN's sign and payload are not part of the arithmetic)
            np.testing.assert_array_equal(got["c"][base:base + n], f["c"], err_msg=w + " coefficients")
            np.testing.assert_array_equal(got["xy_r"][R * lo:R * (lo + m), col], evals[key], err_msg=w + " samples")
            continue
        assert same(got["c"][base:base + n], f["c"]), w + " coefficients"
        assert same(got["xy_r"][R * lo:R * (lo + m), col], evals[key]), w + " samples"


@pytest.mark.parametrize("R", [1, 2, 10])
@pytest.mark.parametrize("m", [4, 5, 9, 23, 64, 129, 300])
def test_single_clip_matches_the_oracle(m, R):
    xy = clip_of(m, extra=("nan_23", "const_23") if m == 23 else ("const_64",) if m == 64 else ())
    off = offsets([m])
    got = run(xy, off, R)
    assert got["xy_r"].shape == (R * m, 36)
    np.testing.assert_array_equal(got["off_out"], R * off)
    check_clip(got, xy, 0, 0, R, "%d frames, R = %d" % (m, R))
    assert same(got["x"], prepare_unsmoothed(got["xy_r"], R * off)), "x is not p3d_clips_prepare(xy_r, smooth = 0)"
    again = run(xy, off, R, with_info=False)                                 # info = NULL: the workspace's record
    for k in ("x", "xy_r", "off_out", "info", "t", "c"):
        assert same(got[k], again[k]), "%s differs between two identical calls" % k


BRANCH_TRACKS = {"A": "move_23", "A_from_a_stage_1_polynomial": "move_4", "B": "move_300", "B_many_knots": "jumpy_64",
                 "C": "lowmotion_1000", "D": "const_64", "iteration_limit": "ier3_27"}


@pytest.mark.parametrize("branch", sorted(BRANCH_TRACKS))
def test_each_branch_alone(branch):
    """A clip whose 36 columns are one golden track of the branch (the 1000-frame one keeps its state
    in the workspace, not in LDS)."""
    name = BRANCH_TRACKS[branch]
    i = NAMES.index(name)
    y = GOLD["y_%d" % i]
    want = dict(A=0, B=1, C=2, D=3)[branch[0]] if branch[0] in "ABCD" else 1
    assert int(GOLD["meta"][i, 5]) == want
    f = oracle(y)
    if branch == "C":
        assert f["n"] > f["n1"]
    if branch == "iteration_limit":
        assert f["ier1"] == 3 and f["ier2"] == 3         # (stage 2 converges and leaves the ier it was handed, as scipy reports it)
    if "polynomial" in branch:
        assert f["ier1"] == -2
    xy = np.ascontiguousarray(np.repeat(y[:, None], 36, axis=1))
    got = run(xy, offsets([len(y)]), 2)
    check_clip(got, xy, 0, 0, 2, branch)


BATCH = [4, 9, 129, 300]


def test_batch_carries_the_single_clip_bits():
    lens = BATCH
    off, R = offsets(lens), 2
    clips = [clip_of(m) for m in lens]
    xy = np.concatenate(clips)
    got = run(xy, off, R)
    np.testing.assert_array_equal(got["off_out"], R * off)
    for s, (a, m) in enumerate(zip(off[:-1], lens)):
        one = run(clips[s], offsets([m]), R)
        assert same(one["xy_r"], got["xy_r"][R * a:R * (a + m)]), "xy_r of clip %d" % s
        assert same(one["x"], got["x"][R * a:R * (a + m)]), "x of clip %d" % s
        assert same(one["info"][0], got["info"][s]), "info of clip %d" % s
        base = 36 * (a + 4 * s)
        assert same(one["t"], got["t"][base:base + 36 * (m + 4)]) and same(one["c"], got["c"][base:base + 36 * (m + 4)])
    check_clip(got, clips[1], int(off[1]), 1, R, "batch")


@pytest.mark.parametrize("table", range(5))
def test_wrong_device_offsets_change_rows_only(table):
    """A wrong device copy of the offsets changes rows only: the guards around every output and the
    workspace (checked in run) are unchanged."""
    N, R = sum(BATCH), 2
    xy = np.concatenate([clip_of(m) for m in BATCH])
    out = run(xy, offsets(BATCH), R, off_dev=WRONG(N)[table])
    assert out["xy_r"].shape == (R * N, 36)


def test_nan_column_mask():
    """A column holding a NaN follows the arithmetic: scipy's recorded mask, and the x rows' with it."""
    i = NAMES.index("nan_23")
    xy = clip_of(23, extra=("nan_23",))
    for R in (1, 2, 10):
        got = run(xy, offsets([23]), R)
        np.testing.assert_array_equal(np.isnan(got["xy_r"][:, 35]), np.isnan(GOLD["v%d_%d" % (R, i)]))
        assert np.isfinite(got["xy_r"][:, :35]).all()
        np.testing.assert_array_equal(got["info"][0, 35], [int(v) for v in GOLD["meta"][i, [1, 3, 2, 4]]] + [0])
