"""GPU tests of the device noise (csrc/p3d_vae_noise.h k_vae_noise, p3d_vae_add_noise,
data_handler.add_noise_device / Dataset / load_3d_data) and of the drivers that train on it
(vae_filter.py, 3d_pose_vae_filter_kin.py --device_noise) against tests/vae_noise_oracle.py.

Bounds.  The noised-row set and the chosen joints are integer work on one Philox block: exactly the
oracle's.  Clean rows, the window form against the plain one, chunked calls, in place, a replayed
graph: bit for bit.  A noised element x + (e noise + offset) [+ j joint_scale] differs from the
oracle's only through the device's logf / sinf / cosf in e and j, which tests/test_gpu_vae.py bounds
at EPS_ULPS_BOUND float32 spacings of the oracle's normal: the tolerance is that bound scaled by
`noise` (and by `joint_scale` on the joint's columns) plus two spacings of the result for the two
float32 roundings (the product-sum and the sum with x) that a perturbed e can move.
"""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import vae_noise_oracle as no
from top_vae_3d_pose import data_handler

pytestmark = pytest.mark.gpu

# tests/test_gpu_vae.py: 4 x the worst deviation of k_vae_eps from the oracle's stream measured on an
# MI355X, in float32 spacings of the oracle's value (restated, not widened)
EPS_ULPS_BOUND = 4 * 4.0
SEED = (5 << 32) | 1234567
Z_BOUND = 5.0
HERE = os.path.dirname(os.path.abspath(__file__))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def noised(x, **kw):
    kw.setdefault("seed", SEED)
    kw.setdefault("ctr", 3)
    return data_handler.add_noise_device(x, [1, 1], **kw)


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def _spacing(a):
    return np.spacing(np.maximum(np.abs(a), np.float32(1e-30))).astype(np.float64)


@pytest.mark.parametrize("width", [12, 48, 240])
def test_plain_form_against_the_oracle(width):
    worst = 0.0
    for B in (1, 5, 63, 65, 200):
        x = np.random.default_rng(width + B).standard_normal((B, width)).astype(np.float32)
        ref, mask, jid, e, j = no.noise_stream(x, SEED, 3, row0=7, noise_3d=[1, 1])
        xd = dev(x)
        got = noised(xd, row0=7).cpu().numpy()
        np.testing.assert_array_equal(xd.cpu().numpy(), x)                     # (the source is left alone)
        got_mask = np.any(got.view(np.uint32) != x.view(np.uint32), axis=1)
        np.testing.assert_array_equal(got_mask, mask)
        np.testing.assert_array_equal(got[~mask].view(np.uint32), x[~mask].view(np.uint32))
        if not mask.any():
            continue
        tol = EPS_ULPS_BOUND * _spacing(e) * np.float64(np.float32(no.NOISE)) + 2 * _spacing(ref)
        rows = np.nonzero(mask)[0]
        for k in range(3):
            tol[rows, jid[rows] + k] += EPS_ULPS_BOUND * _spacing(j[rows, k]) * np.float64(data_handler.joint_scale([1, 1]))
        dev_in_tol = (np.abs(got.astype(np.float64) - ref) / tol)[mask]
        worst = max(worst, float(dev_in_tol.max()))
        assert dev_in_tol.max() <= 1.0, (width, B, float(dev_in_tol.max()))
        # the chosen joint, read off directly: what the device added beyond the element noise is
        # large on the oracle's three columns and nothing (to rounding) anywhere else
        elem = x + (e * np.float32(no.NOISE) + np.float32(no.NOISE_OFFSET))
        rest = np.abs(got.astype(np.float64) - elem)
        cols = np.arange(width)[None, :]
        on = (cols >= jid[:, None]) & (cols < jid[:, None] + 3)
        assert rest[mask[:, None] & ~on].max() <= 1e-4
        assert (np.where(on, rest, 0.0).max(axis=1)[mask] > 1e-3).all()
    print("k_vae_noise, width %d: worst deviation %.3f of the tolerance" % (width, worst))


def test_window_form_equals_the_plain_form_on_the_materialised_windows():
    rows, d, width = 40, 48, 144
    table = np.random.default_rng(40).standard_normal((rows, d)).astype(np.float32)
    starts = np.array([0, rows - 3, -5, rows + 9, 17, 17, 17, 30, 29, 28, 27, 3, 0, rows - 3, 36, 38, 1, 2] +
                      list(range(37, -1, -1)) + [5] * 70, np.int64)
    assert len(starts) > 64 and starts.min() < 0 and starts.max() > rows - 3
    cl = np.clip(starts, 0, rows - 3)
    win = table.reshape(-1)[(cl * d)[:, None] + np.arange(width)[None, :]]
    td = dev(table)
    a = noised(td, starts=dev(starts), width=width, row0=11)
    b = noised(dev(win), row0=11)
    assert a.shape == (len(starts), width) and torch.equal(a, b)
    mask, _ = no.row_decisions(len(starts), width, SEED, 3, row0=11)
    assert mask.any() and not mask.all()
    np.testing.assert_array_equal(np.any(bits(a) != win.view(np.uint32), axis=1), mask)
    np.testing.assert_array_equal(td.cpu().numpy(), table)


def test_rows_are_keyed_by_their_global_index():
    x = dev(np.random.default_rng(1).standard_normal((164, 48)).astype(np.float32))
    full = noised(x)
    assert torch.equal(full[100:], noised(x[100:].contiguous(), row0=100))
    assert torch.equal(full, noised(x))                                         # two identical calls
    m0 = (full != x).any(dim=1)
    assert not torch.equal(m0, (noised(x, ctr=4) != x).any(dim=1))
    assert not torch.equal(m0, (noised(x, seed=SEED + 1) != x).any(dim=1))
    assert not torch.equal(m0, (noised(x, seed=SEED + (1 << 32)) != x).any(dim=1))   # (the key's high word)


def test_a_call_past_2_20_rows_equals_its_chunks():
    n = (1 << 20) + 77
    x = torch.randn((n, 12), device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    full = noised(x, row0=5)
    lo = noised(x[:1 << 20], row0=5)
    hi = noised(x[1 << 20:], row0=5 + (1 << 20))
    assert torch.equal(full[:1 << 20], lo) and torch.equal(full[1 << 20:], hi)
    share = float((full != x).any(dim=1).double().mean())
    assert abs(share - no.P_NOISED) < Z_BOUND * np.sqrt(no.P_NOISED * (1 - no.P_NOISED) / n)
    # the window form through the same split
    starts = torch.randint(0, 100, (n,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    w_full = noised(x, starts=starts, width=36)
    assert torch.equal(w_full[1 << 20:], noised(x, starts=starts[1 << 20:].contiguous(), width=36, row0=1 << 20))


def test_in_place_and_a_captured_graph():
    x = dev(np.random.default_rng(3).standard_normal((300, 48)).astype(np.float32))
    want = noised(x)
    y = x.clone()
    assert noised(y, out=y) is y and torch.equal(y, want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out = torch.zeros_like(x)
    with torch.cuda.stream(side):
        noised(x, out=out)
    torch.cuda.synchronize()
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        noised(x, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    x.mul_(2.0)                       # the graph reads the source as it stands at the replay
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, noised(x))


def test_non_finite_rows():
    x = np.random.default_rng(4).standard_normal((200, 48)).astype(np.float32)
    mask, _ = no.row_decisions(200, 48, SEED, 3)
    on, off = np.nonzero(mask)[0], np.nonzero(~mask)[0]
    for rows in (on, off):
        x[rows[0]] = np.nan
        x[rows[1]] = np.inf
        x[rows[2]] = -np.inf
        x[rows[3], 5] = np.nan        # one poisoned element: the rest of the row is noised as ever
    got = noised(dev(x)).cpu().numpy()
    assert np.isnan(got[on[0]]).all() and (got[on[1]] == np.inf).all() and (got[on[2]] == -np.inf).all()
    assert np.isnan(got[on[3], 5]) and np.isfinite(np.delete(got[on[3]], 5)).all()
    np.testing.assert_array_equal(got[off].view(np.uint32), x[off].view(np.uint32))
    sound = np.ones(200, bool)
    sound[on[:3]] = False             # (NaN + y may keep NaN's bits; +-inf + y keeps them)
    np.testing.assert_array_equal(np.any(got.view(np.uint32) != x.view(np.uint32), axis=1)[sound], mask[sound])


@pytest.mark.parametrize("width", [48, 144])
def test_device_statistics(width):
    n = 1 << 16
    x = torch.randn((n, width), device="cuda", generator=torch.Generator(device="cuda").manual_seed(width))
    out = noised(x, ctr=9)
    mask, jid = no.row_decisions(n, width, SEED, 9)
    z, m = no.statistics(x.cpu().numpy(), out.cpu().numpy(), [1, 1], jid=jid)
    print("device, width %d: %d noised rows, z scores %s" % (width, m, z))
    assert m == int(mask.sum())
    assert all(abs(v) <= Z_BOUND for v in z.values()), z


def test_dataset():
    data = np.random.default_rng(6).standard_normal((203, 48)).astype(np.float32)
    ds = data_handler.Dataset(data, batch_size=64, metadata="meta", seed=SEED, ctr0=1, ctr_step=2)
    assert len(ds) == 3 and ds.shape == (203, 48) and ds.metadata == "meta"
    np.testing.assert_array_equal(ds.data.cpu().numpy(), data)
    assert torch.equal(ds.data_noised, data_handler.add_noise_device(ds.data, seed=SEED, ctr=1))
    assert sum(1 for _ in ds) == 3
    np.random.seed(8)
    ds.on_epoch_end(new_noise=True)
    assert torch.equal(ds.data_noised, data_handler.add_noise_device(ds.data, seed=SEED, ctr=3))
    assert not np.array_equal(ds.indexes, np.arange(203)) and sorted(ds.indexes) == list(range(203))
    seen = []
    for i, (xn, xt) in enumerate(ds):              # every noised row with its own clean row
        idx = ds.indexes[i * 64:(i + 1) * 64]
        np.testing.assert_array_equal(xt.cpu().numpy(), data[idx])
        assert torch.equal(xn, ds.data_noised[torch.from_numpy(idx).cuda()])
        assert xn.is_contiguous() and xn.shape == (64, 48)
        seen += list(idx)
    assert len(seen) == len(set(seen)) == 192
    kept = ds.data_noised.clone()
    ds.on_epoch_end()                              # no new noise: the draw stays
    assert torch.equal(ds.data_noised, kept) and ds.draws == 2
    ds.on_epoch_end(new_noise=True)
    assert torch.equal(ds.data_noised, data_handler.add_noise_device(ds.data, seed=SEED, ctr=5))


def _load(name, fname):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(HERE), "3d-pose-baseline_amd", fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _archives(tmp_path):
    """Synthetic H3.6M archives and the settings of tests/test_gpu_vae_seq.py's driver test."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from synth_cameras import write_h36m_archives
    tree, camsp = str(tmp_path / "h36m.npz"), str(tmp_path / "cameras.npz")
    write_h36m_archives(tree, camsp, np.random.default_rng(31), ["Walking", "Directions"], frames=400, sh=False)
    cfg = tmp_path / "train.yml"
    cfg.write_text("train:\n  step_log: 2000\n  learning_rate: 0.0001\n  likelihood_factor: 100.0\n"
                   "  kcs_factor: 0.02\n  dkl_factor: 1.0\n")
    return ["--camera_frame", "--action", "Walking", "--data_dir", tree, "--cameras_path", camsp,
            "--linear_size", "128", "--num_layers", "1", "--residual", "--batch_norm", "--cfg_file", str(cfg),
            "--train_dir", str(tmp_path / "vae"), "--epochs", "2", "--seed", "3"]


def test_vae_filter_driver_trains_on_device_noise(tmp_path):
    import predict_3dpose
    argv = _archives(tmp_path)
    drv = _load("vae_filter_driver", "vae_filter.py")
    np.random.seed(5)
    model, hist = drv.train(argv, read_from_config=True)
    f = drv.ENV.FLAGS
    assert f.learning_rate == 1e-4 and model.input_size == 48 and model.get_step()[0] == 2 * len(model.data_train)
    for k in ("loss_train", "loss_test", "error_pred", "error_noised"):
        assert len(hist[k]) == 2 and np.isfinite(np.asarray(hist[k])).all(), k
    print("train loss per epoch", hist["loss_train"], "test ELBO", hist["loss_test"])
    print("error noised", hist["error_noised"], "error pred", hist["error_pred"])
    assert hist["loss_train"][1].sum() < hist["loss_train"][0].sum()
    saved = drv.weights_path() + ".npz"
    assert saved == os.path.join(drv.ENV.TRAIN_DIR, "vae", "last_model_weights.npz")
    assert os.path.isfile(os.path.join(drv.ENV.TRAIN_DIR, "vae", "train.cfg"))
    with np.load(saved) as z:
        assert sorted(z.files) == sorted(n for n, _, _ in model.param_table)
        for (n, _, _), w in zip(model.param_table, model.get_weights()):
            np.testing.assert_array_equal(z[n], w)
    # the counter scheme: the test split's draw e is ctr = 1 + 2 e over the split's own rows, and
    # epoch e's batches are the first floor(n / B) B of the order after e shuffles -- replayed here
    # from the same np.random seed: the split's permutation, then per epoch end one shuffle of the
    # train indices and one of the test indices
    d = predict_3dpose.load_data(drv._base().lifter_flags(f))
    np.random.seed(5)
    train, test, meta = data_handler.split_3d_data(d)
    np.testing.assert_array_equal(model.data_test.data.cpu().numpy(), test)
    np.testing.assert_array_equal(model.data_train.data.cpu().numpy(), train)
    assert model.data_test.metadata.mean is not None and meta._fields == model.data_test.metadata._fields
    B, itr, ite = f.batch_size, np.arange(len(train)), np.arange(len(test))
    nb = len(test) // B
    assert nb >= 1 and len(model.data_train) == len(train) // B
    for e in range(2):
        noisy, mask, _, _, _ = no.noise_stream(test, f.seed, 1 + 2 * e, noise_3d=f.noise_3d)
        assert mask.any()
        sq = np.square(noisy.astype(np.float64) - test.astype(np.float64))
        want = np.mean([sq[ite[b * B:(b + 1) * B]].mean() for b in range(nb)])
        np.testing.assert_allclose(hist["error_noised"][e], want, rtol=1e-5, atol=0)
        np.random.shuffle(itr)
        np.random.shuffle(ite)
    np.testing.assert_array_equal(model.data_test.indexes, ite)
    assert model.data_train.draws == model.data_test.draws == 3
    model.close()
    for flag in ("--noised_sample", "--sample"):
        with pytest.raises(NotImplementedError):
            drv.train(argv + [flag], read_from_config=True)


def test_kin_driver_with_device_noise_draws_no_host_noise(tmp_path):
    import predict_3dpose
    argv = _archives(tmp_path) + ["--device_noise"]
    kin = _load("pose_vae_filter_kin_noise", "3d_pose_vae_filter_kin.py")
    np.random.seed(5)
    model, hist = kin.train(argv, read_from_config=True)
    state = np.random.get_state()
    f = kin.ENV.FLAGS
    assert f.device_noise and model.input_size == 144 and model.get_step()[0] > 0
    for k, v in hist.items():
        assert len(v) == 2 and np.isfinite(np.asarray(v)).all(), k
    print("train loss per epoch", hist["loss_train"], "test ELBO per epoch", hist["loss_test"])
    assert hist["loss_train"][1].sum() < hist["loss_train"][0].sum()
    model.close()
    # np.random after the run: what a run that drew only the two permutations leaves
    np.random.seed(5)
    d = predict_3dpose.load_data(kin._base().lifter_flags(f))
    tr, _ = data_handler.load_dataset_3d_seq(d, seq_len=kin.SEQ_LEN)
    for _ in range(2):
        np.random.permutation(len(tr["starts"]))
    ours = np.random.get_state()
    assert state[0] == ours[0] and state[2:] == ours[2:]
    np.testing.assert_array_equal(state[1], ours[1])
    assert not kin.ENV.setup(argv=argv[:-1]).device_noise          # (off by default)
