"""GPU tests of the VAE pose filter (csrc/p3d_vae.h, top_vae_3d_pose/) against tests/vae_oracle.py.

Bounds: forward values 2e-5 + 2e-5 |ref| (the project's MLP bound vs the float64 oracle), loss
vectors 1e-5 relative, gradients 1e-3 of each tensor's largest entry, integer models bit for bit
(tests/vae_exact.py proves them exact), five teacher-forced training steps 5e-5 on the weights.
"""
import numpy as np
import pytest
import torch

import vae_exact as ve
import vae_oracle as vo
from top_vae_3d_pose import models

pytestmark = pytest.mark.gpu

SHAPES = {
    "default": vo.DEFAULT_SHAPE,
    "in144": (144, (40, 32), 24, (32, 40), 48),     # the three-frame variant's input
    "edge": (48, (8,), 8, (24,), 48),               # every width 8 mod 16 somewhere: MFMA tile padding
    "out40": (48, (40, 32), 24, (32, 40), 40),      # no KCS term
}
BATCHES = (1, 16, 17, 64, 65, 200, 1000)
GRAD_BATCHES = (17, 64, 200, 1000)
LR = 1e-3


def factors_of(shape):
    return (100.0, 0.02, 1.0) if shape[4] == 48 else (100.0, 0.0, 1.0)    # train.yml's factors


def rand_params(shape, seed):
    P = vo.init_params(shape, seed)
    rng = np.random.default_rng(seed + 1)
    for k in P:
        if k.endswith("/bias"):
            P[k] = (0.1 * rng.standard_normal(P[k].shape)).astype(np.float32)
    return P


_models, _cases = {}, {}


def model_of(name):
    """One device model per shape, shared by the read-only tests (weights rand_params(shape, 3))."""
    if name not in _models:
        shape = SHAPES[name]
        m = models.VAE(shape[0], shape[2], shape[1], shape[3], shape[4], max_batch=1024, seed=5)
        m.set_weights(rand_params(shape, 3))
        _models[name] = m
    return _models[name]


def case_of(name, B):
    """Inputs and the float64 oracle's forward / loss / backward at (shape, B), computed once."""
    if (name, B) not in _cases:
        shape = SHAPES[name]
        rng = np.random.default_rng(100 * B + len(name))
        x = rng.standard_normal((B, shape[0])).astype(np.float32)
        t = rng.standard_normal((B, shape[4])).astype(np.float32)
        eps = rng.standard_normal((B, shape[2])).astype(np.float32)
        P = rand_params(shape, 3)
        c = vo.forward(P, shape, x, eps)
        terms = vo.row_terms(c, t)
        g, _ = vo.backward(P, shape, c, t, factors_of(shape))
        _cases[(name, B)] = dict(x=x, t=t, eps=eps, c=c, terms=terms, loss=vo.loss3(terms, factors_of(shape)), g=g)
    return _cases[(name, B)]


def close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref) - (2e-5 + 2e-5 * np.abs(ref))
    assert err.max() <= 0, (what, float(np.abs(got - ref).max()))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_vs_oracle(name, B):
    m, k = model_of(name), case_of(name, B)
    o = m.forward_device(k["x"], eps=k["eps"], target=k["t"], want=("y", "mean", "log_var", "z"))
    for key in ("y", "mean", "log_var", "z"):
        close(o[key].cpu().numpy(), k["c"][key], key)
    close(o["row_terms"].cpu().numpy(), k["terms"], "row_terms")
    loss = m.loss_device(k["x"], k["t"], factors_of(SHAPES[name]), eps=k["eps"]).cpu().numpy()
    np.testing.assert_allclose(loss, k["loss"], rtol=1e-5, atol=0)
    # only what was asked for is written: y alone equals the full call's y
    y = m.forward_device(k["x"], eps=k["eps"])["y"]
    assert torch.equal(y, o["y"])


@pytest.mark.parametrize("B", GRAD_BATCHES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_gradients_vs_oracle(name, B):
    m, k = model_of(name), case_of(name, B)
    loss = m.compute_gradients(k["x"], k["t"], factors_of(SHAPES[name]), eps=k["eps"]).cpu().numpy()
    np.testing.assert_allclose(loss, k["loss"], rtol=1e-5, atol=0)
    g = m.grads()
    assert sorted(g) == sorted(k["g"])
    for n, ref in k["g"].items():
        err = float(np.abs(g[n] - ref).max())
        print("grad", name, B, n, "err %.3g of max %.3g" % (err, np.abs(ref).max()))
        assert err <= 1e-3 * np.abs(ref).max(), (n, err, float(np.abs(ref).max()))


def test_kcs_factor_needs_48_outputs():
    m, k = model_of("out40"), case_of("out40", 17)
    with pytest.raises(ValueError):
        m.compute_gradients(k["x"], k["t"], (100.0, 0.02, 1.0), eps=k["eps"])
    with pytest.raises(ValueError):
        m.forward_device(k["x"][:, :40])


@pytest.mark.parametrize("B", ve.EXACT_BATCHES)
def test_integer_model_bit_exact(B):
    """y, mean, z, the KCS row terms and every gradient of the integer model equal the oracle bit
    for bit: in the one-launch form (B <= 64) and through the per-block partials, the second run of
    each over a NaN-filled gradient buffer and workspace."""
    k = ve.exact_case(B)
    shape = vo.DEFAULT_SHAPE
    m = models.VAE(shape[0], shape[2], shape[1], shape[3], shape[4], max_batch=B, seed=1)
    m.set_weights(k["P"])
    o = m.forward_device(k["x"], eps=k["eps"], target=k["t"], want=("y", "mean", "z"))
    for key in ("y", "mean", "z"):
        np.testing.assert_array_equal(o[key].cpu().numpy(), k[key], err_msg=key)
    np.testing.assert_array_equal(o["row_terms"][:, 1].cpu().numpy(), k["kcs"])
    for form in ((0, 1) if B <= 64 else (1,)):
        m.set_form(form)
        for run in range(2):
            m.compute_gradients(k["x"], k["t"], k["factors"], eps=k["eps"])
            g = m.grads()
            for n, ref in k["grads"].items():
                np.testing.assert_array_equal(g[n], ref, err_msg="%s form %d run %d" % (n, form, run))
            m.flat("grads").fill_(float("nan"))
            m.flat("workspace").fill_(float("nan"))
    m.close()


def _fresh(P, form=0):
    shape = vo.DEFAULT_SHAPE
    m = models.VAE(shape[0], shape[2], shape[1], shape[3], shape[4], max_batch=64, seed=1)
    m.set_weights(P)
    m.set_form(form)
    return m


def _state(m):
    mm, vv = m.slots()
    return dict(zip([n for n, _, _ in m.param_table], m.get_weights())), mm, vv


def _same(a, b, what):
    for part_a, part_b, tag in zip(a, b, ("w", "m", "v")):
        for n in part_a:
            np.testing.assert_array_equal(part_a[n], part_b[n], err_msg="%s %s %s" % (what, tag, n))


def test_forms_agree_and_graph_replays():
    """B = 64 over 4 steps: the one-launch step == p3d_vae_grad + the stand-alone reduce / Adam ==
    the partials form of the step == a captured graph of the 4 one-launch steps, bit for bit."""
    shape = vo.DEFAULT_SHAPE
    P = rand_params(shape, 8)
    rng = np.random.default_rng(77)
    xs = torch.from_numpy(rng.standard_normal((4, 64, 48)).astype(np.float32)).cuda()
    ts = torch.from_numpy(rng.standard_normal((4, 64, 48)).astype(np.float32)).cuda()
    es = torch.from_numpy(rng.standard_normal((4, 64, 24)).astype(np.float32)).cuda()
    f = factors_of(shape)
    one, two, part, graph = _fresh(P), _fresh(P), _fresh(P, form=1), _fresh(P)
    losses = []
    for s in range(4):
        losses.append(one.train_step_device(xs[s], ts[s], f, LR, eps=es[s]).cpu().numpy().copy())
        two.compute_gradients(xs[s], ts[s], f, eps=es[s])
        two.adam_apply(LR)
        lp = part.train_step_device(xs[s], ts[s], f, LR, eps=es[s]).cpu().numpy()
        np.testing.assert_array_equal(lp, losses[-1])
    torch.cuda.synchronize()
    assert one.get_step()[0] == two.get_step()[0] == part.get_step()[0] == 4
    ref = _state(one)
    _same(_state(two), ref, "grad + adam_apply")
    _same(_state(part), ref, "partials form")
    assert any(np.abs(ref[0][n] - P[n]).max() > 0 for n in P)
    # the captured graph: warm up on the capture stream, restore the state, capture, replay once
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    lg = torch.zeros((4, 3), device="cuda")
    with torch.cuda.stream(side):
        graph.train_step_device(xs[0], ts[0], f, LR, eps=es[0], loss_out=lg[0])
    torch.cuda.synchronize()
    graph.set_weights(P)
    graph.flat("adam_m").zero_()
    graph.flat("adam_v").zero_()
    graph.set_step(0, 0.9, 0.999)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for s in range(4):
            graph.train_step_device(xs[s], ts[s], f, LR, eps=es[s], loss_out=lg[s])
    g.replay()
    torch.cuda.synchronize()
    assert graph.get_step()[0] == 4
    _same(_state(graph), ref, "graph")
    np.testing.assert_array_equal(lg.cpu().numpy(), np.stack(losses))
    for m in (one, two, part, graph):
        m.close()


def test_optimizer_elementwise_and_five_steps_track_oracle():
    """Per step, from the device's own state before it (teacher-forced): Keras Adam in float64 on the
    device's own gradient reproduces m, v and the new weight (the bounds of
    test_optimizer_elementwise_on_device_gradients), and the float64 oracle's whole step (its own
    gradient) lands within 5e-5 of the device's new weights."""
    shape = vo.DEFAULT_SHAPE
    P = rand_params(shape, 12)
    m = _fresh(P)
    f = factors_of(shape)
    rng = np.random.default_rng(5)
    f64, f32 = np.float64, np.float32
    omb1, omb2 = f64(f32(1.0) - f32(0.9)), f64(f32(1.0) - f32(0.999))    # the device's float32 constants
    aeps = f64(f32(1e-7))
    u = 2.0 ** -24
    for step in range(5):
        x = rng.standard_normal((64, 48)).astype(f32)
        t = rng.standard_normal((64, 48)).astype(f32)
        eps = rng.standard_normal((64, 24)).astype(f32)
        w0, m0, v0 = _state(m)
        s0, b1p, b2p = m.get_step()
        assert s0 == step
        m.train_step_device(x, t, f, LR, eps=eps)
        torch.cuda.synchronize()
        g = m.grads()
        w1, m1, v1 = _state(m)
        alpha = f64(LR) * np.sqrt(1.0 - f64(b2p)) / (1.0 - f64(b1p))
        gref, _ = vo.backward(w0, shape, vo.forward(w0, shape, x, eps), t, f)
        for n in w0:
            gn, mo, vo_ = g[n].astype(f64), m0[n].astype(f64), v0[n].astype(f64)
            mr = mo + (gn - mo) * omb1
            vr = vo_ + (gn * gn - vo_) * omb2
            em = 4 * u * (np.abs(mo) + np.abs(gn - mo) * omb1 + np.abs(mr))
            ev = 4 * u * (np.abs(vo_) + (gn * gn + np.abs(vo_)) * omb2 + np.abs(vr))
            assert np.all(np.abs(m1[n] - mr) <= em), (step, n, "m")
            assert np.all(np.abs(v1[n] - vr) <= ev), (step, n, "v")
            upd = (m1[n].astype(f64) * alpha) / (np.sqrt(v1[n].astype(f64)) + aeps)
            wr = w0[n].astype(f64) - upd
            tol = np.spacing(np.abs(wr).astype(f32)).astype(f64) + 1e-6 * np.abs(upd)
            assert np.all(np.abs(w1[n].astype(f64) - wr) <= tol), (step, n, "w")
            # the oracle's own step from the same state
            wo, _, _ = vo.adam_apply(w0[n].astype(f64), mo, vo_, gref[n], LR, step + 1)
            err = float(np.abs(w1[n] - wo).max())
            assert err < 5e-5, (step, n, err)
    m.close()


def test_internal_eps_equals_the_eps_kernel():
    m, k = model_of("default"), case_of("default", 200)
    a = m.forward_device(k["x"], eps=None, ctr=7, want=("y", "z"))
    e = m.eps_device(200, ctr=7)
    b = m.forward_device(k["x"], eps=e, want=("y", "z"))
    assert torch.equal(a["z"], b["z"]) and torch.equal(a["y"], b["y"])
    assert not torch.equal(e, m.eps_device(200, ctr=8))
    # rows are keyed by their global index
    assert torch.equal(m.eps_device(164, ctr=7)[100:], m.eps_device(64, ctr=7, row0=100))


# Largest deviation of k_vae_eps from the oracle's stream, in units of the oracle value's float32
# spacing: the device's logf / sinf / cosf against float64 functions rounded to float32.  OCML's
# documented ULP bounds are not available in the build environment, so the bound is 4 x the worst
# deviation measured once on an MI355X over 2^16 rows x 24 columns (MEASUREMENTS.md, "VAE filter").
EPS_ULPS_MEASURED = 4.0
EPS_ULPS_BOUND = 4 * EPS_ULPS_MEASURED


def test_eps_stream_vs_oracle_and_moments():
    m = model_of("default")
    n = 1 << 16
    e = m.eps_device(n, ctr=3).cpu().numpy()
    ref = vo.eps_stream(m.seed, 3, 0, n, 24)
    ulps = np.abs(e.astype(np.float64) - ref) / np.spacing(np.maximum(np.abs(ref), np.float32(1e-30)))
    print("eps stream: worst deviation %.2f ulps of the oracle value" % ulps.max())
    assert ulps.max() <= EPS_ULPS_BOUND, float(ulps.max())
    # sanity: standard normal moments (5 sigma of the estimators) and no repeated Philox block
    cnt = e.size
    assert abs(e.mean()) < 5 / np.sqrt(cnt)
    assert abs(e.var() - 1.0) < 5 * np.sqrt(2.0 / cnt)
    assert len(np.unique(np.ascontiguousarray(e).reshape(-1, 4).view(np.uint64), axis=0)) == cnt // 4


def test_pose3dvae_equals_the_oracles_composition():
    """Lifter then filter on the device: out_3d against the lifter's oracle (the serve tests' bound),
    out_vae against the filter's oracle applied to the device's out_3d (the MLP bound)."""
    import linear_model
    from oracle import ref_mlp
    cfg = ref_mlp.Cfg(linear_size=128, num_layers=1, residual=True, batch_norm=True)
    st = ref_mlp.init_state(cfg, seed=5, bn_seed=6)
    lifter = linear_model.LinearModel(128, 1, True, True, False, 64, 1e-3, "/tmp/p3d_vae_pose", seed=7)
    lifter.set_weights({**st.params, **st.moving})
    pv = models.Pose3DVae(24, [40, 32], [32, 40], pose3d=lifter, max_batch=256, seed=3)
    P = rand_params(vo.DEFAULT_SHAPE, 21)
    pv.vae.set_weights(P)
    rng = np.random.default_rng(2)
    x = rng.standard_normal((150, 32)).astype(np.float32)
    eps = rng.standard_normal((150, 24)).astype(np.float32)
    out_3d, out_vae = pv(torch.from_numpy(x).cuda(), training=False, eps=eps)
    ref3d, _ = ref_mlp.forward(st, x, False, 1.0, 0, 0, 0)
    d = np.abs(out_3d.cpu().numpy() - ref3d)
    assert (d <= 5e-5 + 5e-5 * np.abs(ref3d)).all(), float(d.max())
    close(out_vae.cpu().numpy(), vo.forward(P, vo.DEFAULT_SHAPE, out_3d.cpu().numpy(), eps)["y"], "out_vae")
    with pytest.raises(ValueError):
        pv(torch.zeros((4, 48), device="cuda"))
    with pytest.raises(ValueError):
        pv(torch.from_numpy(x).cuda(), eps=eps[:10])
    for kw in ("use_2d", "use_effnet_ouptut", "pred_bones"):
        with pytest.raises(NotImplementedError):
            models.Pose3DVae(24, [40, 32], [32, 40], pose3d=lifter, **{kw: True})
    pv.close()
    lifter.close()


def test_train_runs_two_epochs_and_the_test_elbo_falls(tmp_path):
    """3d_pose_vae_filter.train() on synthetic H3.6M archives: the frozen lifter restored from a
    predict_3dpose.train checkpoint (--load), two epochs, the test ELBO falls, the weights are saved
    under the Keras names; the lifter is left as the checkpoint had it."""
    import importlib.util
    import os
    import sys
    import predict_3dpose
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "golden"))
    from synth_cameras import write_h36m_archives
    tree, camsp = str(tmp_path / "h36m.npz"), str(tmp_path / "cameras.npz")
    write_h36m_archives(tree, camsp, np.random.default_rng(31), ["Walking", "Directions"], frames=400, sh=False)
    np.random.seed(5)
    data = ["--camera_frame", "--action", "Walking", "--data_dir", tree, "--cameras_path", camsp]
    net = ["--linear_size", "128", "--num_layers", "1", "--residual", "--batch_norm"]
    lflags = predict_3dpose.build_parser().parse_args(
        data + net + ["--epochs", "1", "--dropout", "0.5", "--learning_rate", "1e-3", "--train_dir", str(tmp_path / "exp")])
    lifter = predict_3dpose.train(lflags)
    step, lw = lifter.get_step()[0], lifter.get_weights()
    lifter.close()
    spec = importlib.util.spec_from_file_location(
        "pose_vae_filter", os.path.join(os.path.dirname(here), "3d-pose-baseline_amd", "3d_pose_vae_filter.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    # the reference's own settings (src/train.yml): lr 1e-4, factors 100 / 0.02 / 1.  The archive's poses
    # are random and its test subjects have other cameras, so what carries over to the test set is the
    # early, slow descent of the likelihood term -- at 1e-3 the filter already fits the training
    # subjects in its second epoch and the test ELBO turns (measured: 140.5 -> 146.5)
    cfg = tmp_path / "train.yml"
    cfg.write_text("train:\n  step_log: 2000\n  learning_rate: 0.0001\n  likelihood_factor: 100.0\n"
                   "  kcs_factor: 0.02\n  dkl_factor: 1.0\n")
    model, hist = drv.train(data + net + ["--epochs", "2", "--cfg_file", str(cfg), "--train_dir", str(tmp_path / "vae"),
                                          "--load", str(step), "--lifter_dir", predict_3dpose.train_dir_for(lflags)],
                            read_from_config=True)
    assert drv.ENV.FLAGS.learning_rate == 1e-4 and drv.ENV.FLAGS.likelihood_factor == 100.0
    for k, v in model.pose3d.get_weights().items():
        np.testing.assert_array_equal(v, lw[k], err_msg=k)
    assert len(hist["loss_test"]) == 2 and np.isfinite(hist["loss_test"]).all()
    print("test ELBO per epoch", hist["loss_test"], "errors", hist["error_3d_out"], hist["error_vae_out"])
    assert hist["loss_test"][1].sum() < hist["loss_test"][0].sum()
    assert model.vae.get_step()[0] > 0
    saved = os.path.join(drv.ENV.TRAIN_DIR, "3d_vae", "last_model_weights.npz")
    with np.load(saved) as z:
        assert sorted(z.files) == sorted(n for n, _ in vo.param_names(vo.DEFAULT_SHAPE))
        for (n, _, _), w in zip(model.vae.param_table, model.vae.get_weights()):
            np.testing.assert_array_equal(z[n], w)
    with pytest.raises(ValueError):
        drv.train(data + net + ["--epochs", "1", "--load", str(step + 1), "--lifter_dir", str(tmp_path)])
    model.close()
    model.pose3d.close()
