"""A whole OpenPose clip on the GPU (include/p3d.h: p3d_clip_prepare / p3d_clip_finish /
p3d_clip_lift; src/openpose_3dpose_sandbox.py:140-227, 317-417) against tests/clip_oracle.py,
bit for bit: float64 on both sides, the same operation order."""
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
import clip_oracle  # noqa: E402
import data_pipeline as dp  # noqa: E402
import data_utils  # noqa: E402
import linear_model  # noqa: E402
import openpose_frontend as of  # noqa: E402
from oracle import ref_frontend, ref_mlp  # noqa: E402

C = int(_p3d.lib().p3d_clip_chunk())
USE2, _ = data_utils.dimension_sets(2)
USE3, IGN3 = data_utils.dimension_sets(3)
GOLD = os.path.join(HERE, "golden", "clip_goldens.npz")


def assert_same_bits(got, want, what=""):
    """Equal values (NaN == NaN) and equal signs of zero."""
    got, want = np.asarray(got), np.asarray(want)
    np.testing.assert_array_equal(got, want, err_msg=what)
    if got.dtype.kind == "f":
        ok = ~np.isnan(want)
        np.testing.assert_array_equal(np.signbit(got[ok]), np.signbit(want[ok]), err_msg=what + " (sign of zero)")


def dev(a, dtype=torch.float64):
    return dp.as_device(np.ascontiguousarray(a), dtype)


def work_for(n):
    nbytes = int(_p3d.lib().p3d_clip_workspace(n))
    return torch.empty(max(1, nbytes // 8), dtype=torch.float64, device="cuda"), nbytes


def prepare(xy, smooth, mean2, std2):
    n = xy.shape[0]
    d_xy, m2, s2, u2 = dev(xy), dev(mean2), dev(std2), dp._dims(USE2, 64, "t")
    x = torch.full((n, len(USE2)), 7.0, dtype=torch.float32, device="cuda")
    xy_s = torch.full((n, 36), 7.0, dtype=torch.float64, device="cuda")
    work, nbytes = work_for(n)
    p = _p3d.ptr
    _p3d.check(_p3d.lib().p3d_clip_prepare(p(d_xy), n, int(smooth), p(m2), p(s2), p(u2), len(USE2), p(x), p(xy_s),
                                           p(work), nbytes, _p3d.stream_handle()), "p3d_clip_prepare")
    torch.cuda.synchronize()
    return xy_s.cpu().numpy(), x.cpu().numpy()


def finish(y, xy_s, mean3, std3, cache):
    n = y.shape[0]
    d_y, d_xy, m3, s3, u3 = dev(y, torch.float32), dev(xy_s), dev(mean3), dev(std3), dp._dims(USE3, 96, "t")
    poses = torch.full((n, 96), 7.0, dtype=torch.float64, device="cuda")
    src = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    work, nbytes = work_for(n)
    p = _p3d.ptr
    _p3d.check(_p3d.lib().p3d_clip_finish(p(d_y), n, p(d_xy), p(m3), p(s3), p(u3), len(USE3), 96, int(cache), p(poses),
                                          p(src), p(work), nbytes, _p3d.stream_handle()), "p3d_clip_finish")
    torch.cuda.synchronize()
    return poses.cpu().numpy(), src.cpu().numpy()


def crafted_clip(n, seed):
    """Raw keypoints with ~30 % dropped coordinates and, where the clip is long enough, the cases
    the hold must get right (columns 0-6; the other columns are random)."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(40.0, 900.0, (n, 36))
    xy[rng.random((n, 36)) < 0.3] = 0.0
    xy[:, 0] = 0.0                                   # zero from position 0 on: stays zero
    if n >= 9:
        xy[:, 1:7] = rng.uniform(40.0, 900.0, (n, 6))
        xy[n - 6:, 2] = 0.0                          # a zero run over the last four frames
        xy[n // 2, 3] = np.nan                       # a NaN: not zero, kept
        xy[2:8, 5] = -0.0                            # medians of -0.0 past position 0: held
        xy[0:6, 6] = -0.0                            # a -0.0 median AT position 0: kept with its sign
    if n >= 3 * C + 5:
        xy[C - 10:3 * C + 3, 1] = 0.0                # a zero run over two whole chunks, ending mid-chunk
        xy[2 * C - 2:2 * C + 3, 4] = 0.0             # a short run across one chunk boundary
    return xy


@pytest.fixture(scope="module")
def stats2():
    rng = np.random.default_rng(31)
    return rng.uniform(200, 600, 64), rng.uniform(50, 150, 64)


@pytest.mark.parametrize("n", [1, 9, 10, C - 1, C, C + 1, 3 * C + 5])
@pytest.mark.parametrize("smooth", [1, 0])
def test_prepare_matches_oracle(n, smooth, stats2):
    mean2, std2 = stats2
    xy = crafted_clip(n, 100 + n)
    want = clip_oracle.smooth(xy, smooth=bool(smooth))
    xy_s, x = prepare(xy, smooth, mean2, std2)
    assert_same_bits(xy_s, want, "xy_s")
    want_x = dp.normalize(of.map_frames(want), mean2, std2, USE2, out_dtype=torch.float32).cpu().numpy()
    assert_same_bits(x, want_x, "x")
    if smooth and n >= 9:                            # the crafted cases are really there
        assert not want[:, 0].any()
        assert np.all(want[n - 4:, 2] == want[n - 5, 2]) and want[n - 5, 2] != 0
        assert np.isnan(want[n // 2, 3])
        assert np.signbit(want[0, 6]) and want[0, 6] == 0 and np.all(np.signbit(want[:3, 6]))
        assert want[3, 5] == want[0, 5] != 0
    if smooth and n >= 3 * C + 5:
        assert want[C - 1, 1] != 0 and np.all(want[C:3 * C, 1] == want[C - 1, 1])
        assert want[2 * C, 4] == want[2 * C - 1, 4] != 0


def test_prepare_matches_reference_goldens(stats2):
    mean2, std2 = stats2
    with np.load(GOLD, allow_pickle=False) as z:
        for c in z["cases"]:
            xy_s, _ = prepare(z["xy_" + c], 1, mean2, std2)
            assert_same_bits(xy_s, z["sm_" + c], c)


def stats3(kind, seed=41):
    """3D statistics whose swapped z' (dimensions 3j + 1) are mixed in sign, all above 10000
    (_min = min(10000, ...) bites) or all negative (_max = max(0, ...) bites)."""
    rng = np.random.default_rng(seed)
    mean3, std3 = rng.uniform(-400, 400, 96), rng.uniform(30, 300, 96)
    z = np.arange(96) % 3 == 1
    if kind == "high":
        mean3[z], std3[z] = rng.uniform(10500, 12000, z.sum()), rng.uniform(1, 5, z.sum())
    elif kind == "negative":
        mean3[z], std3[z] = rng.uniform(-700, -100, z.sum()), rng.uniform(1, 5, z.sum())
    exact = int([d for d in USE3 if d % 3 == 2][0])           # an exported y (no offset): value = y itself
    mean3[exact], std3[exact] = 0.0, 1.0
    return mean3, std3, list(USE3).index(exact)


def crafted_outputs(n, kind, seed):
    """Network rows whose frames fail (an x far below -1000) where `fail` says, plus a frame whose
    minimum is exactly -1000, one just below it and one with a NaN.  Every other value stays above
    -1000: |y| <= 1 keeps x'' >= -300 - 400 - 230, z'' >= -900 and y' >= -700."""
    rng = np.random.default_rng(seed)
    mean3, std3, exact_u = stats3(kind)
    y = rng.uniform(-1, 1, (n, len(USE3))).astype(np.float32)
    xy_s = rng.uniform(400, 700, (n, 36))
    xdim = list(USE3).index(int([d for d in USE3 if d % 3 == 0][0]))
    fail = np.zeros(n, bool)
    # the failing prefix: position 0; kind "negative": no good frame until past a chunk boundary
    lead = 1 if kind != "negative" else (C + 3 if n > C + 8 else 3)
    fail[:lead] = True
    run = None
    if n >= 3 * C + 5:                               # a failing run across two chunk boundaries
        run = (2 * C - 3, 3 * C + 2) if kind == "negative" else (C - 3, 3 * C + 2)
        fail[run[0]:run[1]] = True
    exact, nan, below = lead, lead + 1, lead + 2
    fail[below] = True
    y[fail, xdim] = -100.0                           # x <= -100 * 30 + 400 + 70 < -1000
    y[exact, exact_u] = -1000.0                      # a minimum of exactly -1000: kept
    y[below, exact_u] = np.nextafter(np.float32(-1000.0), np.float32(-np.inf))   # the next float32: fails
    y[nan, 3] = np.nan                               # a NaN minimum: kept
    return y, xy_s, mean3, std3, fail, exact, lead, run


@pytest.mark.parametrize("n", [10, C + 1, 3 * C + 5])
@pytest.mark.parametrize("kind", ["mixed", "high", "negative"])
@pytest.mark.parametrize("cache", [1, 0])
def test_finish_matches_oracle(n, kind, cache):
    y, xy_s, mean3, std3, fail, exact, lead, run = crafted_outputs(n, kind, 7 * n)
    un = clip_oracle.unnormalize(y, mean3, std3, USE3)
    want, want_src = clip_oracle.post(un, xy_s, cache_on_fail=bool(cache))
    poses, src = finish(y, xy_s, mean3, std3, cache)
    np.testing.assert_array_equal(src, want_src)
    assert_same_bits(poses, want, "poses")
    check_crafted(n, kind, cache, un, xy_s, want, want_src, fail, exact, lead, run)


def check_crafted(n, kind, cache, un, xy_s, want, want_src, fail, exact, lead, run):
    """The crafted cases are really there (properties of the oracle's result alone)."""
    zq = un[:, 1::3]
    if kind == "high":
        assert np.nanmin(zq) > 10000
    if kind == "negative":
        assert np.nanmax(zq) < 0
    if not cache:
        np.testing.assert_array_equal(want_src, np.arange(n))
        return
    np.testing.assert_array_equal(want_src != np.arange(n), fail)
    assert np.all(want_src[:lead] == -1) and not want[:lead].any()
    if run:
        assert not fail[run[0] - 1] and np.all(want_src[run[0]:run[1]] == run[0] - 1)
    own = clip_oracle.post(un, xy_s, cache_on_fail=False)[0]
    assert own[exact].min() == -1000.0 and want_src[exact] == exact
    assert np.isnan(own[exact + 1]).any() and want_src[exact + 1] == exact + 1


def model_setup(seed=3):
    rng = np.random.default_rng(seed)
    cfg = ref_mlp.Cfg(linear_size=1024, num_layers=2, residual=True, batch_norm=True)
    st = ref_mlp.init_state(cfg, seed=seed, bn_seed=seed + 1)
    m = linear_model.LinearModel(1024, 2, True, True, False, 64, 1e-3, "/tmp/p3d_clip", seed=11)
    m.set_weights({**st.params, **st.moving})
    s = dict(mean2=rng.uniform(200, 600, 64), std2=rng.uniform(50, 150, 64),
             mean3=rng.uniform(-400, 400, 96), std3=rng.uniform(30, 300, 96))
    # an exported x that the network does not predict sits at -900: a frame fails (x + spine_x - 630
    # < -1000) exactly where its smoothed spine_x is below 530, with every input in the usual range
    s["mean3"][int([d for d in IGN3 if d % 3 == 0][0])] = -900.0
    return st, m, s


def clip_for_model(n, seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(100, 900, (n, 36))
    xy[rng.random((n, 36)) < 0.25] = 0.0
    xy[:, 2:4] = rng.uniform(540, 700, (n, 2))
    xy[10:16, 2] = 450.0                             # spine_x below 530: failing frames
    xy[0:5, 2] = 450.0                               # ... and from position 0
    return xy


@pytest.mark.parametrize("n", [23, 64 + 5])
def test_clip_lifter_equals_the_chain(n):
    """ClipLifter.lift_clip == clip_oracle.smooth -> openpose_frontend.lift on the same tile
    boundaries -> clip_oracle.post, bit for bit; and the network's rows within the front end's
    bound (tests/test_gpu_frontend.py) of the fp64 oracle on the smoothed frames."""
    st, m, s = model_setup()
    assert m.max_batch == 64
    xy = clip_for_model(n, n)
    for cache in (True, False):
        cl = of.ClipLifter(m, s["mean2"], s["std2"], USE2, s["mean3"], s["std3"], IGN3, max_frames=n + 3,
                           cache_on_fail=cache)
        poses, xy_s, src = cl.lift_clip(xy)
        want_s = clip_oracle.smooth(xy)
        assert_same_bits(xy_s, want_s, "xy_s")
        tiles = []
        for r in range(0, n, m.max_batch):
            e = torch.from_numpy(of.map_frames(want_s[r:r + m.max_batch])).cuda()
            out = torch.empty((e.shape[0], 96), dtype=torch.float64, device="cuda")
            of.lift(m, e, cl.m2, cl.s2, cl.u2, cl.m3, cl.s3, cl.u3, out=out)
            tiles.append(out.cpu().numpy())
        un = np.concatenate(tiles)
        want, want_src = clip_oracle.post(un, want_s, cache_on_fail=cache)
        np.testing.assert_array_equal(src, want_src)
        assert_same_bits(poses, want, "poses")
        if cache:
            assert want_src[0] == -1 and (want_src != np.arange(n)).sum() >= 4
        norm = cl.network_rows(n).cpu().numpy().astype(np.float64)
        _, ref_norm = ref_frontend.lift_frames(st, want_s, s["mean2"], s["std2"], USE2, s["mean3"], s["std3"], IGN3)
        err = np.abs(norm - ref_norm)
        assert np.all(err <= 2e-5 + 2e-5 * np.abs(ref_norm)), err.max()
        assert_same_bits(un[:, USE3], norm.astype(np.float32) * s["std3"][USE3] + s["mean3"][USE3], "unnormalised rows")
        m.check_errors()
    m.close()


def test_clip_lift_graph_replay_equals_eager():
    st, m, s = model_setup(5)
    n = 64 + 5
    xy = clip_for_model(n, 77)
    cl = of.ClipLifter(m, s["mean2"], s["std2"], USE2, s["mean3"], s["std3"], IGN3, max_frames=n)
    poses, xy_s, src = cl.lift_clip(xy)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cl.lift_device(n, True)
    torch.cuda.current_stream().wait_stream(side)
    cl.dout.fill_(3.0)
    cl.dxy.fill_(3.0)
    cl.dsrc.fill_(-9)
    graph.replay()
    torch.cuda.synchronize()
    assert_same_bits(cl.dout.cpu().numpy()[:n], poses)
    assert_same_bits(cl.dxy.cpu().numpy()[:n], xy_s)
    np.testing.assert_array_equal(cl.dsrc.cpu().numpy()[:n], src)
    m.check_errors()
    del graph
    m.close()


def test_argument_errors():
    lib = _p3d.lib()
    ERR = _p3d.P3D_ERR_ARG
    n = 16
    f64 = lambda k: torch.zeros(k, dtype=torch.float64, device="cuda")   # noqa: E731
    xy, xy_s, poses, mean, std = f64(n * 36), f64(n * 36), f64(n * 96), f64(96), f64(96) + 1
    x = torch.zeros(n * 32, dtype=torch.float32, device="cuda")
    y = torch.zeros(n * 48, dtype=torch.float32, device="cuda")
    u = torch.arange(48, dtype=torch.int32, device="cuda")
    work, nbytes = work_for(n)
    p, st = _p3d.ptr, _p3d.stream_handle()

    def prep(N, smooth=1, xy_p=p(xy), w=p(work), wb=nbytes):
        return lib.p3d_clip_prepare(xy_p, N, smooth, p(mean), p(std), p(u), 32, p(x), p(xy_s), w, wb, st)

    def fin(N=9, D3=96, y_p=p(y), w=p(work), wb=nbytes):
        return lib.p3d_clip_finish(y_p, N, p(xy_s), p(mean), p(std), p(u), 48, D3, 1, p(poses), None, w, wb, st)

    for N in range(2, 9):
        assert prep(N) == ERR and b"min 9 frames" in lib.p3d_last_error()
    assert prep(0) == ERR and prep((1 << 20) + 1) == ERR
    assert prep(9, xy_p=None) == ERR and prep(9, xy_p=p(xy_s)) == ERR
    assert prep(9, w=None) == ERR
    assert prep(9, wb=nbytes - 1) == ERR and b"workspace" in lib.p3d_last_error()
    assert prep(9) == 0 and prep(5, smooth=0) == 0 and prep(1) == 0
    assert fin(D3=48) == ERR and b"96" in lib.p3d_last_error()
    assert fin(y_p=None) == ERR and fin(w=None) == ERR and fin(wb=8) == ERR and fin(N=(1 << 20) + 1) == ERR
    assert fin() == 0
    torch.cuda.synchronize()
    assert lib.p3d_clip_lift(None, p(xy), 9, 1, p(mean), p(std), p(u), 32, p(mean), p(std), p(u), 48, 96, 1, p(xy_s),
                             p(poses), None, p(work), nbytes, st) == ERR
    with pytest.raises(ValueError):
        _p3d.check(prep(4), "p3d_clip_prepare")
    assert lib.p3d_clip_workspace(1 << 20) > 0 and C >= 8


def test_clip_lift_rejects_mismatched_model_and_short_workspace():
    st_, m, s = model_setup(6)
    cl = of.ClipLifter(m, s["mean2"], s["std2"], USE2, s["mean3"], s["std3"], IGN3, max_frames=32)
    lib, p = _p3d.lib(), _p3d.ptr
    args = lambda U2=32, wb=cl.work_bytes: (m._h, p(cl.din), 20, 1, p(cl.m2), p(cl.s2), p(cl.u2), U2, p(cl.m3),   # noqa: E731
                                            p(cl.s3), p(cl.u3), 48, 96, 1, p(cl.dxy), p(cl.dout), p(cl.dsrc),
                                            cl.work_ptr, wb, m.stream())
    assert lib.p3d_clip_lift(*args(U2=16)) == _p3d.P3D_ERR_ARG
    assert lib.p3d_clip_lift(*args(wb=int(lib.p3d_clip_workspace(20)))) == _p3d.P3D_ERR_ARG
    with pytest.raises(ValueError):
        cl.lift_clip(np.ones((5, 36)))
    with pytest.raises(ValueError):
        cl.lift_clip(np.ones((33, 36)))
    m.close()


def test_sandbox_driver_end_to_end(tmp_path):
    """The driver on a directory of frame files (synthetic statistics, fresh weights): both export
    files, the reference's nesting, the 2D export equal to the reference's own smoothing."""
    import json
    import openpose_3dpose_sandbox as sandbox
    with np.load(GOLD, allow_pickle=False) as z:
        raw, want_s = z["raw_body25_23"], z["sm_body25_23"]
    frames = tmp_path / "json"
    frames.mkdir()
    for i, row in enumerate(raw):
        with open(frames / ("clip_%012d_keypoints.json" % i), "w") as f:
            json.dump({"people": [{"pose_keypoints_2d": [float(v) for v in row]}]}, f)
    base = ["--synthetic", "--residual", "--batch_norm", "--max_batch", "128", "--verbose", "0",
            "--pose_estimation_json", str(frames), "--out_dir", str(tmp_path / "maya")]
    p3, p2 = sandbox.main(base)
    three, two = json.load(open(p3)), json.load(open(p2))
    assert sorted(three, key=int) == sorted(two, key=int) == [str(i) for i in range(23)]
    got_s = np.array([[two[str(i)][str(j)]["translate"] for j in range(18)] for i in range(23)]).reshape(23, 36)
    assert_same_bits(got_s, want_s)
    poses = np.array([[three[str(i)][str(j)]["translate"] for j in range(32)] for i in range(23)])
    assert poses.shape == (23, 32, 3) and np.isfinite(poses).all()
    for flag in ("--interpolation", "--write_gif"):
        with pytest.raises(SystemExit):
            sandbox.main(base + [flag])
