"""GPU tests of sample()'s numbers (src/predict_3dpose.py:447-577): p3d_sample_world against the
composition of the existing kernels it fuses (bit for bit) and against the numpy oracle
(tests/sample_oracle.py), and predict_3dpose.main(["--sample", ...]) end to end over the archive
form of the H3.6M tree."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-pose-baseline_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import data_pipeline as dp  # noqa: E402
import data_utils  # noqa: E402
import predict_3dpose  # noqa: E402
import sample_oracle as so  # noqa: E402
from synth_cameras import synth_cameras, synth_world_poses, write_h36m_archives  # noqa: E402

# tests/test_oracle_data.py's tolerance for camera_to_world_frame (a host BLAS may order the 3x3
# product differently)
RTOL, ATOL = 1e-12, 1e-9
SIZES = (1, 2, 63, 64, 65, 257)
NMAX = max(SIZES)


def bits(t):
    return t.contiguous().view(torch.int64)


class Case:
    """Shared, read-only inputs: camera-frame poses of NMAX rows, normalised, for U = 48 and 42."""

    def __init__(self):
        rng = np.random.default_rng(41)
        self.rcams, packed, _ = synth_cameras(rng, subjects=(9,))
        self.cams = packed[0]                                     # [4, 21]
        world = synth_world_poses(rng, NMAX)                      # [n, 96] mm
        self.cam_of_row = rng.integers(0, 4, NMAX).astype(np.int32)
        camf = np.empty_like(world)
        for c in range(4):
            R, T = self.rcams[(9, c + 1)][:2]
            m = self.cam_of_row == c
            camf[m] = (R @ (world[m].reshape(-1, 3).T - T)).T.reshape(-1, 96)
        self.root = camf[:, :3].copy()
        centred = camf - np.tile(self.root, (1, 32))
        self.mean = centred.mean(0) + rng.normal(0, 1, 96)
        self.std = centred.std(0) + rng.uniform(1, 2, 96)
        self.use, self.ign, self.yn = {}, {}, {}
        for U in (48, 42):
            use, ign = data_utils.dimension_sets(3, U == 42)
            assert len(use) == U
            self.use[U], self.ign[U] = np.asarray(use), np.asarray(ign)
            self.yn[U] = (centred[:, use] - self.mean[use]) / self.std[use]   # float64

    def yn_of(self, U, dtype):
        return torch.from_numpy(self.yn[U].astype(dtype)).cuda()


@pytest.fixture(scope="module")
def case():
    return Case()


def composed(yn, mean, std, use, cams, cam_of_row, root):
    """The four existing calls sample_world fuses, over the same rows."""
    x = dp.unnormalize(yn, mean, std, use, 96)
    if root is not None:
        x = x + dp.as_device(root).repeat(1, 32)
    pts = x.reshape(-1, 3)
    cm = dp.as_device(cams).reshape(-1, 21)
    if cam_of_row is None:
        w = dp.camera_to_world(pts, cm[0:1])[0].reshape(-1, 96)
    else:
        allc = dp.camera_to_world(pts, cm).reshape(cm.shape[0], -1, 96)    # every camera, every row
        sel = torch.as_tensor(np.asarray(cam_of_row), dtype=torch.int64, device=x.device)
        w = allc[sel, torch.arange(x.shape[0], device=x.device)].contiguous()
    return dp.root_center(w)[0]


@pytest.mark.parametrize("U", [48, 42])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fused_equals_composed_bit_for_bit(case, U, dtype):
    yn_all = case.yn_of(U, dtype)
    for n in SIZES:
        for mixed in (True, False):
            for with_root in (True, False):
                cor = case.cam_of_row[:n] if mixed else None
                root = case.root[:n] if with_root else None
                yn = yn_all[:n].contiguous()
                got = dp.sample_world(yn, case.mean, case.std, case.use[U], case.cams, cor, root)
                want = composed(yn, case.mean, case.std, case.use[U], case.cams, cor, root)
                assert got.shape == (n, 96) and got.dtype == torch.float64
                assert torch.equal(bits(got), bits(want)), (n, mixed, with_root)


def test_unaligned_float32_input_takes_the_scalar_loads(case):
    """A float32 input that is not 16-byte aligned (a view one float into a buffer) runs the
    instance with 4-byte loads: the same bits."""
    n, U = 65, 48
    buf = torch.zeros(n * U + 1, dtype=torch.float32, device="cuda")
    buf[1:] = case.yn_of(U, np.float32)[:n].reshape(-1)
    yn = buf[1:].view(n, U)
    assert yn.data_ptr() % 16 == 4 and yn.is_contiguous()
    got = dp.sample_world(yn, case.mean, case.std, case.use[U], case.cams, case.cam_of_row[:n], case.root[:n])
    want = dp.sample_world(yn.clone(), case.mean, case.std, case.use[U], case.cams, case.cam_of_row[:n], case.root[:n])
    assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("U", [48, 42])
def test_against_the_numpy_oracle(case, U):
    n = NMAX
    yn = case.yn[U].astype(np.float32)
    for with_root in (True, False):
        got = dp.sample_world(yn, case.mean, case.std, case.use[U], case.cams, case.cam_of_row,
                              case.root if with_root else None).cpu().numpy()
        want = np.empty((n, 96))
        for c in range(4):
            R, T = case.rcams[(9, c + 1)][:2]
            m = case.cam_of_row == c
            want[m] = so.world_rows(yn[m], case.mean, case.std, case.ign[U], R, T,
                                    root=case.root[m] if with_root else None)
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
        assert np.abs(got).max() > 100.0        # (millimetres, not zeros)


def test_bad_host_indices_are_refused(case):
    yn = case.yn[48][:4].astype(np.float32)
    with pytest.raises(ValueError, match="camera indices out of range"):
        dp.sample_world(yn, case.mean, case.std, case.use[48], case.cams, [0, 1, 4, 2])
    with pytest.raises(ValueError, match="dimension indices out of range"):
        dp.sample_world(yn, case.mean, case.std, np.arange(49, 97), case.cams)
    with pytest.raises(ValueError, match="cam_of_row has"):
        dp.sample_world(yn, case.mean, case.std, case.use[48], case.cams, [0, 1, 2])
    with pytest.raises(ValueError, match="root must be"):
        dp.sample_world(yn, case.mean, case.std, case.use[48], case.cams, root=np.zeros((3, 3)))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_rows_stay_in_their_row(case, bad):
    n, U = 65, 48
    clean = case.yn[U][:n].astype(np.float32)
    args = (case.mean, case.std, case.use[U], case.cams, case.cam_of_row[:n], case.root[:n])
    ref = dp.sample_world(clean, *args)
    dirty = clean.copy()
    dirty[17, 5] = bad          # one value of one row
    dirty[40, :] = bad          # a whole row
    got = dp.sample_world(dirty, *args)
    want = composed(torch.from_numpy(dirty).cuda(), *args)
    rows = torch.ones(n, dtype=torch.bool, device="cuda")
    rows[[17, 40]] = False
    assert torch.equal(bits(got[rows]), bits(ref[rows]))
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert not bool(torch.isfinite(got[17]).all()) and not bool(torch.isfinite(got[40]).all())
    fin = ~torch.isnan(got)
    assert torch.equal(bits(got[fin]), bits(want[fin]))
    # the same for a root that is not finite
    root = case.root[:n].copy()
    root[3, 1] = bad
    got = dp.sample_world(clean, *args[:5], root)
    want = composed(torch.from_numpy(clean).cuda(), *args[:5], root)
    rows = torch.ones(n, dtype=torch.bool, device="cuda")
    rows[3] = False
    assert torch.equal(bits(got[rows]), bits(ref[rows]))
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and not bool(torch.isfinite(got[3]).any())
    fin = ~torch.isnan(got)
    assert torch.equal(bits(got[fin]), bits(want[fin]))


def test_sample_world_is_capturable(case):
    n, U = 257, 48
    yn1, yn2 = case.yn_of(U, np.float32)[:n].contiguous(), case.yn_of(U, np.float32)[:n].flip(0).contiguous()
    mean, std = dp.as_device(case.mean), dp.as_device(case.std)
    use = dp.as_device(case.use[U].astype(np.int32), torch.int32)
    cams, root = dp.as_device(case.cams), dp.as_device(case.root[:n])
    cor = dp.as_device(case.cam_of_row[:n], torch.int32)
    eager1 = dp.sample_world(yn1, mean, std, use, cams, cor, root)
    eager2 = dp.sample_world(yn2, mean, std, use, cams, cor, root)
    buf, out = yn1.clone(), torch.zeros((n, 96), dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dp.sample_world(buf, mean, std, use, cams, cor, root, out=out)
    torch.cuda.synchronize()
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        dp.sample_world(buf, mean, std, use, cams, cor, root, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(eager1))
    buf.copy_(yn2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(eager2))


def test_a_split_across_2_20_rows_does_not_show(case):
    big, tail, U = (1 << 20) + 65, 65, 48
    assert big > dp.SAMPLE_MAX_ROWS
    gen = torch.Generator(device="cuda").manual_seed(43)
    yn = torch.randn((big, U), dtype=torch.float32, device="cuda", generator=gen)
    root = torch.randn((big, 3), dtype=torch.float64, device="cuda", generator=gen) * 1000.0
    cor = torch.randint(0, 4, (big,), dtype=torch.int32, device="cuda", generator=gen)
    got = dp.sample_world(yn, case.mean, case.std, case.use[U], case.cams, cor, root)
    want = dp.sample_world(yn[-tail:].contiguous(), case.mean, case.std, case.use[U], case.cams,
                           cor[-tail:].contiguous(), root[-tail:].contiguous())
    assert tuple(got.shape) == (big, 96)
    assert torch.equal(bits(got[-tail:]), bits(want))
    # (and the rows on either side of the seam are those of a call that has no seam there)
    lo, hi = dp.SAMPLE_MAX_ROWS - 33, dp.SAMPLE_MAX_ROWS + 33
    seam = dp.sample_world(yn[lo:hi].contiguous(), case.mean, case.std, case.use[U], case.cams,
                           cor[lo:hi].contiguous(), root[lo:hi].contiguous())
    assert torch.equal(bits(got[lo:hi]), bits(seam))


@pytest.mark.parametrize("use_sh", [False, True])
@pytest.mark.parametrize("camera_frame", [True, False])
def test_sample_end_to_end(tmp_path, capsys, camera_frame, use_sh):
    """predict_3dpose.main(["--sample", ...]) over the archive form of the H3.6M tree, a fresh
    seeded model: every key's slice against the oracle, fed the model's own forward output.  (The
    archive holds two actions; --action selects one, the other is a decoy.)"""
    rng = np.random.default_rng(51)
    tree, camsp = str(tmp_path / "h36m.npz"), str(tmp_path / "cameras.npz")
    write_h36m_archives(tree, camsp, rng, ["Sitting", "Walking"], frames=150, sh=use_sh)
    outdir = str(tmp_path / "out")
    argv = ["--data_dir", tree, "--cameras_path", camsp, "--train_dir", str(tmp_path / "exp"),
            "--action", "Walking", "--linear_size", "128", "--num_layers", "1", "--residual", "--batch_norm",
            "--seed", "5", "--sample", "--sample_dir", outdir]
    argv += ["--camera_frame"] if camera_frame else []
    argv += ["--use_sh"] if use_sh else []
    np.random.seed(77)
    keep = predict_3dpose.FLAGS
    try:
        res = predict_3dpose.main(argv)
    finally:
        predict_3dpose.FLAGS = keep
    flags = predict_3dpose.build_parser().parse_args(argv)
    d = predict_3dpose.load_data(flags, with_roots=True)
    keys = list(d["test_set_2d"].keys())
    assert res["keys"] == keys and len(keys) == 2 * 2 * 4      # subjects x sequences x cameras
    lens = [d["test_set_2d"][k].shape[0] for k in keys]
    np.testing.assert_array_equal(res["seq_off"], np.concatenate([[0], np.cumsum(lens)]))
    N = int(res["seq_off"][-1])
    for name, w in (("enc_in", 64), ("dec_out", 96), ("poses3d", 96)):
        assert tuple(res[name].shape) == (N, w) and res[name].dtype == torch.float64 and res[name].is_cuda
    printed = capsys.readouterr().out
    for subj, a, fname in keys:
        assert "Subject: {}, action: {}, fname: {}".format(subj, a, fname) in printed
    assert "drawing is not built" in printed and os.path.join(outdir, "samples.npz") in printed
    # the model's own forward output: the same fresh seeded model over the same rows
    model = predict_3dpose.create_model(None, None, 128, flags)
    assert N <= model.max_batch
    X = np.vstack([d["test_set_2d"][k] for k in keys]).astype(np.float32)
    pred_n = model.forward_device(torch.from_numpy(X).cuda(), False, 1.0).cpu().numpy()
    model.close()
    got = {k: res[k].cpu().numpy() for k in ("enc_in", "dec_out", "poses3d")}
    for i, key2d in enumerate(keys):
        lo, hi = int(res["seq_off"][i]), int(res["seq_off"][i + 1])
        key3d = so.key3d_of(key2d, camera_frame)
        cam = so.the_camera(d["rcams"], key3d) if camera_frame else None
        root = d["test_root_positions"][key3d] if camera_frame else None
        want = so.sample_key(d["test_set_2d"][key2d], d["test_set_3d"][key3d], pred_n[lo:hi], d, camera_frame,
                             cam=cam, root=root)
        for name, w in zip(("enc_in", "dec_out", "poses3d"), want):
            np.testing.assert_allclose(got[name][lo:hi], w, rtol=RTOL, atol=ATOL, err_msg="%s %s" % (name, key2d))
    # the rows the reference draws: the permutation of the LAST key's rows, entries 1 .. 15
    lo = int(res["seq_off"][-2])
    np.random.seed(77)
    idx = so.picked_rows(lens[-1])
    pk = res["picked"]
    assert pk["key"] == keys[-1] and len(idx) == 15
    np.testing.assert_array_equal(pk["idx"], idx)
    for name in ("enc_in", "dec_out", "poses3d"):
        np.testing.assert_array_equal(pk[name], got[name][lo + idx])
    with np.load(os.path.join(outdir, "samples.npz"), allow_pickle=False) as z:
        assert [str(v) for v in z["key"]] == [str(v) for v in keys[-1]]
        np.testing.assert_array_equal(z["idx"], idx)
        for name in ("enc_in", "dec_out", "poses3d"):
            np.testing.assert_array_equal(z[name], pk[name])


def test_sample_synthetic_runs(tmp_path):
    """--synthetic alone works (sequences of any length >= 1; no cameras: plain un-normalisation)."""
    argv = ["--synthetic", "--train_dir", str(tmp_path / "exp"), "--linear_size", "128", "--num_layers", "1",
            "--seed", "3", "--sample"]
    np.random.seed(5)
    keep = predict_3dpose.FLAGS
    try:
        res = predict_3dpose.main(argv)
    finally:
        predict_3dpose.FLAGS = keep
    N = int(res["seq_off"][-1])
    assert tuple(res["poses3d"].shape) == (N, 96) and len(res["picked"]["idx"]) == 15
    assert bool(torch.isfinite(res["poses3d"]).all()) and bool(torch.isfinite(res["dec_out"]).all())
