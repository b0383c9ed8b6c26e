"""GPU tests of the wide VAE filter (in > 256: csrc/p3d_vae_wide.h, the cat / dx forms of
csrc/p3d_vae.h, models.VAE with segments, models.Pose3DVaeCat and the
3d_pose_effnet_2d_vae_filter.py driver) against tests/vae_oracle.py.

Bounds are the project's: forward values 2e-5 + 2e-5 |ref| vs the float64 oracle, loss vectors 1e-5
relative, gradients 1e-3 of each tensor's largest entry, integer models bit for bit
(tests/vae_exact.py proves them exact), five teacher-forced training steps 5e-5 on the weights.
"""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import vae_exact as ve
import vae_oracle as vo
from top_vae_3d_pose import models

pytestmark = pytest.mark.gpu

SHAPES = {
    "wide": (1360, (40, 32), 24, (32, 40), 48),      # [x2d | out_3d | effnet_out]
    "edge264": (264, (8,), 8, (24,), 48),            # the first width past the limit; every padded-tile case
    "max2048": (2048, (40, 32), 24, (32, 40), 40),   # the widest input; no KCS term
}
BATCHES = (1, 17, 64, 65, 200)
# Row-chunk constants of the wide kernels: k_vae_wide_wgrad_adam takes WGRAD_ROUND = 16 rows a round of
# its one chain, the core pass (k_vae_step_dx) works in CORE_BLOCK = 64-row blocks.  17 and 65 are one
# row past each.
WGRAD_ROUND, CORE_BLOCK = 16, 64
GRAD_BATCHES = (WGRAD_ROUND + 1, 64, CORE_BLOCK + 1, 200)
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
    if name not in _models:
        shape = SHAPES[name]
        m = models.VAE(shape[0], shape[2], shape[1], shape[3], shape[4], max_batch=256, seed=5)
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
    print(what, "max |err| %.3g" % float(np.abs(got - ref).max()))
    assert err.max() <= 0, (what, float(np.abs(got - ref).max()))


def test_param_table_and_workspace():
    """Layer 0 sits in the Keras table and the flat buffers like any other tensor, and the workspace
    grows over the narrow formula by no more than h0 and dz0."""
    m = model_of("wide")
    shape = SHAPES["wide"]
    assert [(n, s) for n, s, _ in m.param_table] == vo.param_names(shape)
    assert m.param_table[0][2] == 0 and m.param_table[1][2] == 1360 * 40 and m.param_table[2][2] == 1361 * 40
    P = sum(int(np.prod(s)) for _, s, _ in m.param_table)
    assert m.flat("params").numel() == P == m.flat("grads").numel() == m.flat("adam_m").numel()
    import _p3d
    for B in (1, 64, 65, 256):
        ws = _p3d.lib().p3d_vae_workspace(m._h, B) // 4
        nblk = (B + 63) // 64
        assert ws <= nblk * (P + 4) + 4 + 2 * B * 40
        assert ws >= 2 * B * 40
    # no per-block partial of layer 0: at 2^20 rows the formula stays within 2 B enc0 + the small layers' partials
    big = models.VAE(1360, 24, [40, 32], [32, 40], max_batch=1 << 20, seed=1, init=False)
    ws = _p3d.lib().p3d_vae_workspace(big._h, 1 << 20) // 4
    assert ws <= (1 << 14) * (P - 1361 * 40 + 4) + 4 + 2 * (1 << 20) * 40
    big.close()
    with pytest.raises(ValueError):
        m.filter_sequences(torch.zeros((4, 48), device="cuda"), [0, 4])


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


@pytest.mark.parametrize("B", (16, 64, 128))
@pytest.mark.parametrize("name", ("wide", "edge264"))
def test_integer_model_bit_exact(name, B):
    """y, mean, z, the KCS row terms and every gradient (layer 0's included) of the integer model
    equal the oracle bit for bit, in forms 0 and 1 where B <= 64, the second run of each over a
    NaN-filled gradient buffer and workspace."""
    shape = SHAPES[name]
    k = ve.exact_case(B, shape)
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


def _fresh(shape, P, form=0, max_batch=64):
    m = models.VAE(shape[0], shape[2], shape[1], shape[3], shape[4], max_batch=max_batch, seed=1)
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


@pytest.mark.parametrize("widths,table_rows", (((32, 48, 1280), 300), ((32, 48), 0)), ids=("wide1360", "narrow80"))
def test_cat_equals_the_materialised_input(widths, table_rows):
    """Segments -- the last wide one a (table, idx) pair whose index repeats rows and leaves the table
    once on each side (those read the clamped rows) -- give the bits of the plain call on torch.cat of
    the gathered rows: y, the loss vector, every gradient, and after three training steps the
    weights and both Adam slots."""
    n_in = sum(widths)
    shape = (n_in, (40, 32), 24, (32, 40), 48)
    B = 70
    rng = np.random.default_rng(9)
    dev = torch.device("cuda")
    segs_np = [rng.standard_normal((B, w)).astype(np.float32) for w in widths]
    segs, mat = [], []
    for w, a in zip(widths, segs_np):
        if w == 1280:
            table = torch.from_numpy(rng.standard_normal((table_rows, w)).astype(np.float32)).to(dev)
            idx = rng.integers(0, table_rows, size=B)
            idx[3] = idx[2]
            idx[10], idx[11] = -5, table_rows + 7
            idx = torch.from_numpy(idx.astype(np.int64)).to(dev)
            segs.append((table, idx))
            mat.append(table[idx.clamp(0, table_rows - 1)])
        else:
            segs.append(torch.from_numpy(a).to(dev))
            mat.append(segs[-1])
    x = torch.cat(mat, dim=1).contiguous()
    t = torch.from_numpy(rng.standard_normal((B, 48)).astype(np.float32)).to(dev)
    eps = torch.from_numpy(rng.standard_normal((B, 24)).astype(np.float32)).to(dev)
    P = rand_params(shape, 4)
    f = factors_of(shape)
    a, b = _fresh(shape, P, max_batch=128), _fresh(shape, P, max_batch=128)
    ya = a.forward_device(segs, eps=eps)["y"]
    yb = b.forward_device(x, eps=eps)["y"]
    assert torch.equal(ya, yb) and bool(torch.isfinite(ya).all())
    la = a.loss_device(segs, t, f, eps=eps).clone()
    assert torch.equal(la, b.loss_device(x, t, f, eps=eps))
    la = a.compute_gradients(segs, t, f, eps=eps).clone()
    assert torch.equal(la, b.compute_gradients(x, t, f, eps=eps))
    assert torch.equal(a.flat("grads"), b.flat("grads")) and bool(a.flat("grads").abs().sum() > 0)
    for _ in range(3):
        la = a.train_step_device(segs, t, f, LR, eps=eps).clone()
        assert torch.equal(la, b.train_step_device(x, t, f, LR, eps=eps))
    for which in ("params", "adam_m", "adam_v"):
        assert torch.equal(a.flat(which), b.flat(which)), which
    assert a.get_step()[0] == b.get_step()[0] == 3
    # host-side checks of the segments
    bad = [[segs[0]], [segs[0][:, :28].contiguous()] + segs[1:], [segs[0].double()] + segs[1:],
           [segs[0].cpu()] + segs[1:], [segs[0][:10]] + segs[1:], [segs[0].t().contiguous().t()] + segs[1:]]
    if table_rows:
        bad += [segs[:2] + [(segs[2][0], segs[2][1][:10])], segs[:2] + [(segs[2][0], segs[2][1].int())]]
    for s in bad:
        with pytest.raises(ValueError):
            a.forward_device(s, eps=eps)
    a.close()
    b.close()


def test_forms_agree_and_graph_replays():
    """Shape wide, B = 64 over 4 steps: train_step == grad + adam_apply == form 1 == a captured graph
    of the 4 steps on one stream, bit for bit."""
    shape = SHAPES["wide"]
    P = rand_params(shape, 8)
    rng = np.random.default_rng(77)
    xs = torch.from_numpy(rng.standard_normal((4, 64, shape[0])).astype(np.float32)).cuda()
    ts = torch.from_numpy(rng.standard_normal((4, 64, 48)).astype(np.float32)).cuda()
    es = torch.from_numpy(rng.standard_normal((4, 64, 24)).astype(np.float32)).cuda()
    f = factors_of(shape)
    one, two, part, graph = _fresh(shape, P), _fresh(shape, P), _fresh(shape, P, form=1), _fresh(shape, P)
    three = _fresh(shape, P, form=1)       # grad + adam_apply through the partials form
    losses = []
    for s in range(4):
        losses.append(one.train_step_device(xs[s], ts[s], f, LR, eps=es[s]).cpu().numpy().copy())
        two.compute_gradients(xs[s], ts[s], f, eps=es[s])
        two.adam_apply(LR)
        three.compute_gradients(xs[s], ts[s], f, eps=es[s])
        three.adam_apply(LR)
        lp = part.train_step_device(xs[s], ts[s], f, LR, eps=es[s]).cpu().numpy()
        np.testing.assert_array_equal(lp, losses[-1])
    torch.cuda.synchronize()
    assert one.get_step()[0] == two.get_step()[0] == part.get_step()[0] == three.get_step()[0] == 4
    ref = _state(one)
    _same(_state(two), ref, "grad + adam_apply")
    _same(_state(three), ref, "grad + adam_apply, form 1")
    _same(_state(part), ref, "partials form")
    assert all(np.abs(ref[0][n] - P[n]).max() > 0 for n in P)
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
    for m in (one, two, three, part, graph):
        m.close()


def test_five_steps_track_the_oracles_adam():
    """Five teacher-forced training steps at shape wide: from the device's own state before each
    step, the float64 oracle's whole step lands within 5e-5 of the device's new weights."""
    shape = SHAPES["wide"]
    P = rand_params(shape, 12)
    m = _fresh(shape, P)
    f = factors_of(shape)
    rng = np.random.default_rng(5)
    f64, f32 = np.float64, np.float32
    for step in range(5):
        x = rng.standard_normal((64, shape[0])).astype(f32)
        t = rng.standard_normal((64, 48)).astype(f32)
        eps = rng.standard_normal((64, 24)).astype(f32)
        w0, m0, v0 = _state(m)
        assert m.get_step()[0] == step
        m.train_step_device(x, t, f, LR, eps=eps)
        torch.cuda.synchronize()
        w1, _, _ = _state(m)
        gref, _ = vo.backward(w0, shape, vo.forward(w0, shape, x, eps), t, f)
        worst = 0.0
        for n in w0:
            wo, _, _ = vo.adam_apply(w0[n].astype(f64), m0[n].astype(f64), v0[n].astype(f64), gref[n], LR, step + 1)
            err = float(np.abs(w1[n] - wo).max())
            worst = max(worst, err)
            assert err < 5e-5, (step, n, err)
        print("step", step, "worst weight error %.3g" % worst)
    m.close()


def test_pose3dvaecat_equals_the_oracles_composition():
    """Lifter then the 1360-input filter on the device: out_3d against the lifter's oracle, out_vae
    against the filter's oracle applied to [x, the device's out_3d, features]."""
    import linear_model
    from oracle import ref_mlp
    cfg = ref_mlp.Cfg(linear_size=128, num_layers=1, residual=True, batch_norm=True)
    st = ref_mlp.init_state(cfg, seed=5, bn_seed=6)
    lifter = linear_model.LinearModel(128, 1, True, True, False, 64, 1e-3, "/tmp/p3d_vae_pose_cat", seed=7)
    lifter.set_weights({**st.params, **st.moving})
    pv = models.Pose3DVaeCat(24, [40, 32], [32, 40], use_effnet_ouptut=True, use_2d=True, pose3d=lifter,
                             max_batch=256, seed=3)
    shape = SHAPES["wide"]
    assert pv.vae.input_size == 1360
    P = rand_params(shape, 21)
    pv.vae.set_weights(P)
    rng = np.random.default_rng(2)
    x = rng.standard_normal((150, 32)).astype(np.float32)
    feat = (0.1 * rng.standard_normal((400, 1280))).astype(np.float32)
    idx = rng.permutation(400)[:150].astype(np.int64)
    eps = rng.standard_normal((150, 24)).astype(np.float32)
    F = torch.from_numpy(feat).cuda()
    out_3d, out_vae = pv(torch.from_numpy(x).cuda(), effnet_output=(F, torch.from_numpy(idx).cuda()), eps=eps)
    ref3d, _ = ref_mlp.forward(st, x, False, 1.0, 0, 0, 0)
    d = np.abs(out_3d.cpu().numpy() - ref3d)
    assert (d <= 5e-5 + 5e-5 * np.abs(ref3d)).all(), float(d.max())
    xin = np.concatenate([x, out_3d.cpu().numpy(), feat[idx]], axis=1)
    close(out_vae.cpu().numpy(), vo.forward(P, shape, xin, eps)["y"], "out_vae")
    # a plain [B, 1280] tensor is the same input
    _, out2 = pv(torch.from_numpy(x).cuda(), effnet_output=torch.from_numpy(feat[idx]).cuda(), eps=eps)
    assert torch.equal(out2, out_vae)
    with pytest.raises(ValueError):
        pv(torch.from_numpy(x).cuda(), effnet_output=F[:150, :1272].contiguous(), eps=eps)
    with pytest.raises(ValueError):
        pv(torch.from_numpy(x).cuda(), effnet_output=F[:100], eps=eps)
    with pytest.raises(ValueError):
        pv(torch.from_numpy(x).cuda(), eps=eps)
    with pytest.raises(NotImplementedError):
        models.Pose3DVaeCat(24, [40, 32], [32, 40], pose3d=lifter, pred_bones=True)
    # use_2d alone: the 80-input filter over [x2d, out_3d]
    p2 = models.Pose3DVaeCat(24, [40, 32], [32, 40], use_2d=True, pose3d=lifter, max_batch=256, seed=3)
    s80 = (80, (40, 32), 24, (32, 40), 48)
    P80 = rand_params(s80, 22)
    p2.vae.set_weights(P80)
    o3, ov = p2(torch.from_numpy(x).cuda(), eps=eps)
    close(ov.cpu().numpy(), vo.forward(P80, s80, np.concatenate([x, o3.cpu().numpy()], axis=1), eps)["y"], "out_vae 80")
    p2.close()
    pv.close()
    lifter.close()


def test_driver_trains_two_epochs(tmp_path):
    """3d_pose_effnet_2d_vae_filter.train() on synthetic H3.6M archives and a synthetic feature
    archive: the frozen lifter restored from a predict_3dpose.train checkpoint, two epochs at the
    train.yml settings; histories finite, the mean training loss falls from epoch 1 to epoch 2 (the
    test ELBO is printed only: with random features nothing says it must fall), the lifter unchanged,
    the weights saved under the Keras names."""
    import predict_3dpose
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "golden"))
    from synth_cameras import write_h36m_archives
    from effnet_synth import write_effnet_archive
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
    d = predict_3dpose.load_data(lflags)
    feats = str(tmp_path / "effnet.npz")
    write_effnet_archive(feats, [d["train_set_2d"], d["test_set_2d"]], np.random.default_rng(6))
    spec = importlib.util.spec_from_file_location(
        "pose_effnet_2d_vae_filter", os.path.join(os.path.dirname(here), "3d-pose-baseline_amd",
                                                  "3d_pose_effnet_2d_vae_filter.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    cfg = tmp_path / "train.yml"
    cfg.write_text("train:\n  step_log: 2000\n  learning_rate: 0.0001\n  likelihood_factor: 100.0\n"
                   "  kcs_factor: 0.02\n  dkl_factor: 1.0\n")
    common = data + net + ["--cfg_file", str(cfg), "--train_dir", str(tmp_path / "vae"), "--effnet_outputs_path", feats,
                           "--load", str(step), "--lifter_dir", predict_3dpose.train_dir_for(lflags)]
    model, hist = drv.train(common + ["--epochs", "2", "--use_effb1"], read_from_config=True)
    assert drv.ENV.FLAGS.learning_rate == 1e-4 and drv.ENV.FLAGS.likelihood_factor == 100.0
    for k, v in model.pose3d.get_weights().items():
        np.testing.assert_array_equal(v, lw[k], err_msg=k)
    for key in ("loss_train", "loss_test", "error_3d_out", "error_vae_out"):
        assert len(hist[key]) == 2 and np.isfinite(np.asarray(hist[key], np.float64)).all(), key
    print("train loss per epoch", hist["loss_train"], "test ELBO per epoch", hist["loss_test"],
          "errors", hist["error_3d_out"], hist["error_vae_out"])
    assert hist["loss_train"][1].sum() < hist["loss_train"][0].sum()
    assert model.vae.get_step()[0] > 0 and model.vae.input_size == 1360
    saved = os.path.join(drv.ENV.TRAIN_DIR, "3d_effnet_2d_vae", "last_model_weights.npz")
    assert os.path.isfile(os.path.join(drv.ENV.TRAIN_DIR, "3d_effnet_2d_vae", "train.cfg"))
    with np.load(saved) as z:
        assert sorted(z.files) == sorted(n for n, _ in vo.param_names(SHAPES["wide"]))
        assert z["enc_h_40/kernel"].shape == (1360, 40)
        for (n, _, _), w in zip(model.vae.param_table, model.vae.get_weights()):
            np.testing.assert_array_equal(z[n], w)
    for flag, exc in ((["--train_all"], NotImplementedError), (["--sample"], NotImplementedError),
                      (["--optimizer", "rmsprop"], NotImplementedError)):
        with pytest.raises(exc):
            drv.train(common + ["--epochs", "1"] + flag)
    model.close()
    model.pose3d.close()
