"""CPU tests of the VAE filter's oracle (tests/vae_oracle.py) and of the host side of p3d_vae_*:
the oracle against an independent torch-autograd statement of the same graph, the KCS bone matrix
against a literal per-sample loop, Adam against a scalar loop, the exactness proof of the integer
cases (tests/vae_exact.py), argument validation of p3d_vae_create without a GPU, the flags."""
import ctypes

import numpy as np
import pytest
import torch

import _p3d
import vae_exact as ve
import vae_oracle as vo

SHAPES = [vo.DEFAULT_SHAPE, (144, (40, 32), 24, (32, 40), 48), (48, (8,), 8, (24,), 40)]
FACTORS = [(100.0, 0.02, 1.0), (1.0, 1.0, 1.0), (1.0, 0.0, 0.0), (0.0, 0.5, 3.0)]   # first: train.yml's


def _rand(shape, seed, B=5):
    rng = np.random.default_rng(seed)
    P = vo.init_params(shape, seed)
    for k in P:
        if k.endswith("/bias"):
            P[k] = (0.1 * rng.standard_normal(P[k].shape)).astype(np.float32)
    return (P, rng.standard_normal((B, shape[0])), rng.standard_normal((B, shape[2])),
            rng.standard_normal((B, shape[4])))


def _torch_graph(P, shape, x, eps, t, factors):
    """The reference's graph written with torch ops and autograd (float64): models.py:25-80 and
    losses.py:14-109, the bone matrix built by index arithmetic rather than the oracle's loop."""
    _, enc, lat, dec, out = shape
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in P.items()}
    h = torch.tensor(x)
    for u in enc:
        h = torch.relu(h @ p["enc_h_%d/kernel" % u] + p["enc_h_%d/bias" % u])
    mean = h @ p["mean/kernel"] + p["mean/bias"]
    lv = h @ p["log_varianze/kernel"] + p["log_varianze/bias"]
    z = torch.tensor(eps) * torch.exp(lv * 0.5) + mean
    d = z
    for u in dec:
        d = torch.relu(d @ p["dec_f_%d/kernel" % u] + p["dec_f_%d/bias" % u])
    y = d @ p["dec_f_out/kernel"] + p["dec_f_out/bias"]
    tt = torch.tensor(t)
    dkl = 0.5 * torch.sum(torch.exp(lv) + mean ** 2 - 1.0 - lv, dim=-1)
    like = torch.mean((tt - y) ** 2, dim=-1)
    if out == 48:
        map_i = np.array([1, 2, 3, 1, 5, 6, 1, 8, 9, 10, 9, 12, 13, 9, 15, 16]) - 1     # losses.py:74
        map_j = np.array([2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17]) - 1   # losses.py:75
        sel = torch.tensor((map_i != 0).astype(np.float64))[None, :, None]
        def dirs(a):
            j = a.reshape(a.shape[0], -1, 3)
            return (j[:, map_j - 1] - sel * j[:, map_i - 1]).transpose(1, 2)     # [B, 3, 16]
        bp, bt = dirs(y), dirs(tt)
        phi = bp.transpose(1, 2) @ bp - bt.transpose(1, 2) @ bt
        kcs = phi.abs().sum(dim=(2, 1))
    else:
        kcs = torch.zeros(len(x), dtype=torch.float64)
    loss = torch.stack([factors[0] * like.mean(), factors[1] * kcs.mean(), factors[2] * dkl.mean()])
    loss.sum().backward()
    g = {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in p.items()}
    return dict(y=y.detach().numpy(), mean=mean.detach().numpy(), log_var=lv.detach().numpy(), z=z.detach().numpy(),
                terms=torch.stack([like, kcs, dkl], dim=1).detach().numpy(), loss=loss.detach().numpy(), g=g)


@pytest.mark.parametrize("factors", FACTORS)
@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_matches_torch_autograd(shape, factors):
    if shape[4] != 48:
        factors = (factors[0], 0.0, factors[2])
    P, x, eps, t = _rand(shape, 3)
    ref = _torch_graph(P, shape, x, eps, t, factors)
    c = vo.forward(P, shape, x, eps)
    for k in ("y", "mean", "log_var", "z"):
        assert np.abs(c[k] - ref[k]).max() < 1e-10, k
    terms = vo.row_terms(c, t)
    assert np.abs(terms - ref["terms"]).max() < 1e-10
    assert np.abs(vo.loss3(terms, factors) - ref["loss"]).max() < 1e-10
    g, _ = vo.backward(P, shape, c, t, factors)
    assert sorted(g) == sorted(ref["g"])
    for k in g:
        assert np.abs(g[k] - ref["g"][k]).max() < 1e-7, k


def test_kcs_bone_matrix_matches_the_literal_loop():
    """The per-sample loop of losses.py:85-100, decrements and the `i == 0` quirk included."""
    rng = np.random.default_rng(4)
    pred = rng.standard_normal((3, 48))
    map_i = np.array([1, 2, 3, 1, 5, 6, 1, 8, 9, 10, 9, 12, 13, 9, 15, 16]) - 1
    map_j = np.array([2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17]) - 1
    po = pred.reshape(pred.shape[0], -1, 3)
    dirs = []
    for k in range(po.shape[0]):
        bones = []
        for i, j in zip(map_i, map_j):
            if i == 0:
                bones.append(po[k][j - 1])
                continue
            bones.append(po[k][j - 1] - po[k][i - 1])
        dirs.append(np.stack(bones))
    np.testing.assert_array_equal(vo.bones(pred), np.stack(dirs))
    assert [a for a, p in enumerate(vo.PARENT) if p < 0] == [0, 3, 6]
    # sign(0) = 0: identical poses give a zero gradient, not a NaN
    P, x, eps, _ = _rand(vo.DEFAULT_SHAPE, 9)
    c = vo.forward(P, vo.DEFAULT_SHAPE, x, eps)
    g, dy = vo.backward(P, vo.DEFAULT_SHAPE, c, c["y"], (0.0, 1.0, 0.0))
    assert not dy.any()


def test_adam_matches_a_scalar_loop():
    rng = np.random.default_rng(6)
    w, m, v = rng.standard_normal(7), np.zeros(7), np.zeros(7)
    ws, ms, vs = w.copy(), m.copy(), v.copy()
    for t in range(1, 4):
        g = rng.standard_normal(7)
        w, m, v = vo.adam_apply(w, m, v, g, 1e-3, t)
        lr_t = 1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        for i in range(7):
            ms[i] += (g[i] - ms[i]) * (1 - 0.9)
            vs[i] += (g[i] * g[i] - vs[i]) * (1 - 0.999)
            ws[i] -= lr_t * ms[i] / (np.sqrt(vs[i]) + 1e-7)
        np.testing.assert_allclose(w, ws, rtol=1e-14)
        np.testing.assert_allclose(m, ms, rtol=1e-14)
        np.testing.assert_allclose(v, vs, rtol=1e-14)


@pytest.mark.parametrize("B", ve.EXACT_BATCHES)
def test_integer_cases_are_exact(B):
    """The precondition of tests/test_gpu_vae.py::test_integer_model_bit_exact: float32 and float64
    oracles agree bit for bit, every gradient is exactly representable and every contraction's
    absolute sum stays below 2^23 units (asserted inside exact_case)."""
    k = ve.exact_case(B)
    assert max(k["worst"].values()) < ve.LIMIT
    assert k["y"].dtype == np.float32 and k["kcs"].dtype == np.float32
    assert all(np.abs(g).max() > 0 for n, g in k["grads"].items() if n.endswith("/kernel"))


def test_eps_stream_is_standard_normal_and_keyed_by_row():
    e = vo.eps_stream(5, 3, 0, 4096, 24)
    assert e.dtype == np.float32 and e.shape == (4096, 24)
    assert abs(e.mean()) < 5 / np.sqrt(e.size) and abs(e.var() - 1) < 5 * np.sqrt(2 / e.size)
    np.testing.assert_array_equal(e[100:164], vo.eps_stream(5, 3, 100, 64, 24))
    assert not np.array_equal(e, vo.eps_stream(5, 4, 0, 4096, 24))


def _create(i, enc, lat, dec, out, mb=64):
    h = ctypes.c_void_p()
    e, d = (ctypes.c_int32 * max(len(enc), 1))(*enc), (ctypes.c_int32 * max(len(dec), 1))(*dec)
    rc = _p3d.lib().p3d_vae_create(i, len(enc), e, lat, len(dec), d, out, mb, 1, ctypes.byref(h))
    return rc, _p3d.lib().p3d_last_error().decode()


def test_vae_argument_validation_without_gpu():
    for args, word in [((50, [40, 32], 24, [32, 40], 48), "in must"), ((48, [], 24, [32], 48), "hidden layers"),
                       ((48, [40, 32, 24, 16, 8], 24, [32], 48), "hidden layers"), ((48, [36], 24, [32], 48), "hidden widths"),
                       ((48, [40], 72, [32], 48), "latent"), ((48, [40], 24, [32], 72), "out must"),
                       ((48, [40, 40], 24, [32], 48), "unique"), ((256, [256] * 4, 64, [256] * 4, 64), "LDS")]:
        rc, msg = _create(*args)
        assert rc == _p3d.P3D_ERR_ARG and word in msg, (args, rc, msg)
    assert _create(48, [40], 24, [32], 48, mb=0)[0] == _p3d.P3D_ERR_ARG
    assert _create(48, [40], 24, [32], 48, mb=(1 << 20) + 1)[0] == _p3d.P3D_ERR_ARG
    lib = _p3d.lib()
    assert lib.p3d_vae_forward(None, None, 0, None, 0, None, None, None, None, None, None, None) == _p3d.P3D_ERR_ARG
    f3 = (ctypes.c_float * 3)(1, 1, 1)
    assert lib.p3d_vae_train_step(None, None, None, 64, None, f3, 1e-3, None, None) == _p3d.P3D_ERR_ARG
    assert lib.p3d_vae_eps(1, 0, 0, 64, 22, None, None) == _p3d.P3D_ERR_ARG
    assert lib.p3d_vae_destroy(None) == 0
    if not torch.cuda.is_available():   # a valid shape then fails on the missing device, loudly
        assert _create(48, [40, 32], 24, [32, 40], 48)[0] == 2
        from top_vae_3d_pose import models
        with pytest.raises(_p3d.P3DError):
            models.VAE(48, 24, [40, 32], [32, 40])
        with pytest.raises(ValueError):
            models.VAE(50, 24, [40, 32], [32, 40])


def test_vae_flags_follow_the_reference(tmp_path):
    """Names and defaults of src/top_vae_3d_pose/args_def.py:21-105; a settings file shaped like
    src/train.yml overrides them."""
    from top_vae_3d_pose.args_def import ENVIRON as ENV
    f = ENV.setup(argv=[])
    assert (f.learning_rate, f.batch_size, f.epochs, f.latent_dim, f.enc_dim, f.dec_dim) == (0.001, 64, 200, 24,
                                                                                            [40, 32], [32, 40])
    assert (f.likelihood_factor, f.kcs_factor, f.dkl_factor, f.optimizer, f.step_log) == (1.0, 1.0, 1.0, "adam", 1000)
    assert not f.train_all and f.load == 0 and f.cfg_file == "src/train.yml"
    cfg = tmp_path / "train.yml"
    cfg.write_text("train:\n  step_log: 2000\n  learning_rate: 0.0001\n  # Reconstruction factor loss\n"
                   "  likelihood_factor: 100.0\n  kcs_factor: 0.02\n  dkl_factor: 1.0\n")
    f = ENV.setup(read_from_config=True, argv=["--cfg_file", str(cfg), "--latent_dim", "16"])
    assert (f.step_log, f.learning_rate, f.likelihood_factor, f.kcs_factor, f.dkl_factor) == (2000, 1e-4, 100.0, 0.02, 1.0)
    assert f.latent_dim == 16
    ENV.setup(argv=[])
