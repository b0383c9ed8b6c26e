"""CPU tests of the temporal filter's oracle (tests/vae_seq_oracle.py), of the host plumbing in
top_vae_3d_pose/data_handler.py and of the host side of p3d_vae_seq_*: the batched recurrence
against a literal per-frame loop, the proof that the integer case is exact, the noise against a
row-by-row loop, the sliding windows, the key map, the new symbols and their argument checks."""
import ctypes

import numpy as np
import pytest

import _p3d
import vae_oracle as vo
import vae_seq_oracle as so

IN144 = (144, (40, 32), 24, (32, 40), 48)
EDGE96 = (96, (8,), 8, (24,), 48)


def _rand_params(shape, seed):
    P = vo.init_params(shape, seed)
    rng = np.random.default_rng(seed + 1)
    for k in P:
        if k.endswith("/bias"):
            P[k] = (0.1 * rng.standard_normal(P[k].shape)).astype(np.float32)
    return P


def _case(shape, lens, seed):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(off[-1])
    return (off, rng.standard_normal((N, shape[4])).astype(np.float32),
            rng.standard_normal((N, shape[2])).astype(np.float32), rng.standard_normal((N, shape[4])).astype(np.float32))


@pytest.mark.parametrize("shape", [IN144, EDGE96], ids=["in144", "edge96"])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_batched_oracle_equals_the_literal_loop(shape, dt):
    lens = [1, 2, 3, 9, 0, 5, 4]
    off, pred, eps, tgt = _case(shape, lens, 3)
    P = _rand_params(shape, 3)
    a = so.filter(P, shape, pred, off, eps, target=tgt, dt=dt)
    b = so.filter_literal(P, shape, pred, off, eps, target=tgt, dt=dt)
    # (BLAS may block a matrix product by its batch: rounding noise of the type, nothing more)
    tol = dict(rtol=1e-12, atol=1e-13) if dt is np.float64 else dict(rtol=1e-4, atol=1e-5)
    for k in ("ref", "frame_err", "seq_err"):
        np.testing.assert_allclose(a[k], b[k], err_msg=k, **tol)
    assert a["ref"].dtype == dt
    # frame 0 sees [p0] * seq_len; a one-frame sequence is that frame alone
    L = so.seq_len_of(shape)
    y0 = vo.forward(P, shape, np.tile(pred[0:1], (1, L)), eps[0:1], dt)["y"]
    np.testing.assert_allclose(a["ref"][0:1], y0, **tol)
    # err_pred does not depend on the filter
    np.testing.assert_allclose(a["frame_err"][:, 0], np.mean(np.square(tgt.astype(dt) - pred.astype(dt)), axis=1),
                               rtol=1e-6)


@pytest.mark.parametrize("at", [1, 2, 7])
def test_chunked_oracle_equals_one_pass(at):
    shape = IN144
    lens = [1, 2, 3, 9, 0, 5, 12]
    off, pred, eps, tgt = _case(shape, lens, 4)
    P = _rand_params(shape, 3)
    whole = so.filter(P, shape, pred, off, eps, target=tgt)
    i1, o1, i2, o2 = so.split(off, at)
    assert len(i1) + len(i2) == len(pred) and sorted(np.concatenate([i1, i2])) == list(range(len(pred)))
    st = so.new_state(shape, len(lens))
    a = so.filter(P, shape, pred[i1], o1, eps[i1], target=tgt[i1], state=st)
    assert list(st[1]) == [int(n > 0) for n in lens]
    b = so.filter(P, shape, pred[i2], o2, eps[i2], target=tgt[i2], state=st)
    got = np.zeros_like(whole["ref"])
    got[i1], got[i2] = a["ref"], b["ref"]
    np.testing.assert_array_equal(got, whole["ref"])
    np.testing.assert_allclose(a["seq_err"] + b["seq_err"], whole["seq_err"], rtol=1e-12)


def test_integer_case_is_exact():
    """The precondition of tests/test_gpu_vae_seq.py's integer test: per frame float32 == float64 bit
    for bit, integers, absolute contraction sums below 2^23 (asserted inside exact_case)."""
    k = so.exact_case()
    assert k["ref"].shape == (240, 48) and k["ref"].dtype == np.float32
    assert np.array_equal(k["ref"], np.round(k["ref"]))
    assert 0 < k["max_abs"] < 2.0 ** 10
    assert np.abs(k["pred"]).max() <= 2 and set(np.unique(k["eps"])) <= {-2.0, 0.0, 2.0}
    # the recurrence is live: the refined poses feed back (frame 2 differs from a fresh window's output)
    fresh = vo.forward(k["P"], k["shape"], np.tile(k["pred"][2:3], (1, 3)), k["eps"][2:3])["y"]
    assert not np.array_equal(fresh[0], k["ref"][2])


# ------------------------------------------------------------------ data_handler
def _add_noise_loop(data, noise_3d):
    """data_handler.py:48-84 row by row."""
    data_noised = np.array(data)
    nsamples, points_dim = data.shape
    noise = 0.22108747
    noised_all = np.random.randn(nsamples, points_dim) * noise + 0.0011787938
    joints_idx = np.random.choice(np.arange(points_dim), nsamples)
    noise_single_joint = np.random.randn(nsamples, 3) * (noise + noise_3d[1])
    probs = np.random.randn(nsamples)
    for i in range(nsamples):
        if probs[i] < 0.5:
            continue
        data_noised[i] += noised_all[i]
        jid = joints_idx[i] - joints_idx[i] % 3
        data_noised[i][jid] += noise_single_joint[i][0]
        data_noised[i][jid + 1] += noise_single_joint[i][1]
        data_noised[i][jid + 2] += noise_single_joint[i][2]
    return data_noised


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_add_noise_equals_the_row_loop(dt):
    from top_vae_3d_pose import data_handler as dh
    data = np.random.default_rng(0).standard_normal((257, 144)).astype(dt)
    keep = data.copy()
    np.random.seed(12)
    got = dh.add_noise(data, noise_3d=[1, 0.5])
    after = np.random.rand()
    np.random.seed(12)
    want = _add_noise_loop(data, [1, 0.5])
    assert np.random.rand() == after                     # the same draws were consumed
    assert got.dtype == dt and np.array_equal(got, want)
    assert np.array_equal(data, keep)                    # a copy is noised
    clean = (got == data).all(axis=1)
    assert 0.55 < clean.mean() < 0.85                    # randn() < 0.5: about 69 % stay clean
    changed = (got != data)[~clean]
    assert changed.all()                                 # a noised row is noised everywhere
    # FLAGS.noise_3d is the default
    from top_vae_3d_pose.args_def import ENVIRON as ENV
    assert list(ENV.FLAGS.noise_3d) == [1, 1] and ENV.FLAGS.evaluate is False and ENV.FLAGS.vae_weights is None
    np.random.seed(12)
    a = dh.add_noise(data)
    np.random.seed(12)
    assert np.array_equal(a, _add_noise_loop(data, [1, 1]))


def test_load_dataset_3d_seq_windows():
    from top_vae_3d_pose import data_handler as dh
    rng = np.random.default_rng(2)
    lens = {("S1", "Walking", "a.h5"): 10, ("S1", "Walking", "b.h5"): 3, ("S5", "Eating", "c.h5"): 4,
            ("S5", "Eating", "d.h5"): 1}
    tr = {k: rng.standard_normal((n, 48)) for k, n in lens.items()}
    te = {("S9", "Walking", "e.h5"): rng.standard_normal((6, 48))}
    train, test = dh.load_dataset_3d_seq({"train_set_3d": tr, "test_set_3d": te}, seq_len=3)
    assert train["frames"].dtype == np.float32 and train["frames"].shape == (18, 48)
    assert train["keys"] == list(lens) and list(train["seq_off"]) == [0, 10, 13, 17, 18]
    counts = [int((train["window_key"] == i).sum()) for i in range(4)]
    assert counts == [max(n - 3, 0) for n in lens.values()] == [7, 0, 1, 0]
    assert len(test["starts"]) == 3 and list(test["starts"]) == [0, 1, 2]
    # the reference's generator, word for word
    x_ref, y_ref = [], []
    for k in lens:
        d = tr[k].astype(np.float32)
        for i in range(d.shape[0] - 3):
            x_ref.append(d[i:i + 3].reshape(-1))
            y_ref.append(d[i + 3 - 1])
    x, y = dh.window_x(train), dh.window_y(train)
    assert x.shape == (8, 144) and np.array_equal(x, np.array(x_ref)) and np.array_equal(y, np.array(y_ref))
    assert np.array_equal(x[:, 96:], y)                                 # y is the window's last frame
    # a window is contiguous in the frame array; the last possible window (start n - 3) is dropped
    s = int(train["starts"][6])
    assert s == 6 and np.array_equal(x[6], train["frames"].reshape(-1)[s * 48:(s + 3) * 48])
    assert 7 not in train["starts"][train["window_key"] == 0]
    assert np.array_equal(dh.window_x(train, np.array([7])), np.array(x_ref)[7:8])
    four, _ = dh.load_dataset_3d_seq({"train_set_3d": tr, "test_set_3d": te}, seq_len=4)
    assert [int((four["window_key"] == i).sum()) for i in range(4)] == [6, 0, 0, 0]


def test_get_key3d():
    from top_vae_3d_pose import data_handler as dh
    k = (9, "Walking", "Walking 1.54138969.h5")
    assert dh.get_key3d(k, camera_frame=True) == k
    assert dh.get_key3d(k, camera_frame=False) == (9, "Walking", "Walking 1.h5")
    sh = (9, "Walking", "Walking 1.54138969.h5-sh")
    assert dh.get_key3d(sh, camera_frame=True) == (9, "Walking", "Walking 1.54138969.h5")
    assert dh.get_key3d(sh, camera_frame=False) == (9, "Walking", "Walking 1.h5")
    from top_vae_3d_pose.args_def import ENVIRON as ENV
    assert dh.get_key3d(k) == dh.get_key3d(k, camera_frame=ENV.FLAGS.camera_frame)


# ------------------------------------------------------------------ the library's host side
def _lds(shape, form):
    i, enc, lat, dec, out = shape
    e, d = (ctypes.c_int32 * len(enc))(*enc), (ctypes.c_int32 * len(dec))(*dec)
    return _p3d.lib().p3d_vae_seq_lds_bytes(i, len(enc), e, lat, len(dec), d, out, form)


def test_seq_symbols_and_argument_checks_without_gpu():
    lib = _p3d.lib()
    for name in ("p3d_vae_seq_filter", "p3d_vae_seq_set_form", "p3d_vae_seq_lds_bytes"):
        assert getattr(lib, name) is not None
        assert name in [s[0] for s in _p3d.SIGNATURES]
    rc = lib.p3d_vae_seq_filter(None, None, None, 1, 1, None, 0, 0, None, None, None, None, None, None, None)
    assert rc == _p3d.P3D_ERR_ARG and b"p3d_vae_seq_filter" in lib.p3d_last_error()
    assert lib.p3d_vae_seq_set_form(None, 0) == _p3d.P3D_ERR_ARG


def test_seq_lds_bytes():
    for shape in (IN144, EDGE96):
        sizes = [_lds(shape, form) for form in (0, 1)]
        for n in sizes:
            assert 0 < n <= 160 * 1024, (shape, n)
        # the packed parameters, one tile's activations and the [16, in] state tile at least; and
        # less than the four-area layout of the per-frame kernels
        P = sum(K * N + N for _, K, N in vo.layer_names(shape))
        assert sizes[0] >= 4 * (P + 16 * shape[0])
        i, enc, lat, dec, out = shape
        e, d = (ctypes.c_int32 * len(enc))(*enc), (ctypes.c_int32 * len(dec))(*dec)
        assert sizes[0] < _p3d.lib().p3d_vae_lds_bytes(i, len(enc), e, lat, len(dec), d, out)
    assert _lds((100, (40, 32), 24, (32, 40), 48), 0) == 0        # in is not a multiple of out
    assert _lds((80, (40, 32), 24, (32, 40), 48), 0) == 0
    assert _lds((48, (40, 32), 24, (32, 40), 48), 1) > 0          # seq_len 1 is served
    assert _lds(IN144, 2) == 0
