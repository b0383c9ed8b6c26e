"""The lifter at the model shapes p3d_create accepts beyond the benchmark's (tests/shape_cases.py):
no hidden layer, 3 to 8 blocks, widths that are no multiple of 128, widths under 256 and past the
batch <= 4 chain's and fold's limits -- each on one side of a threshold at which csrc/p3d.hip picks
another kernel or launch form.  The tags the profile reports must equal the expected ones for every
(shape, batch): a form the table was meant to reach but which did not run is a failure.

Bounds.  Integer models: bit for bit (tests/test_shape_cases_oracle.py proves them exact).  Random
weights up to three blocks: the suite's bounds (outputs 5e-5 + 5e-5 |ref|, gradients 1e-3 of each
tensor's largest entry, moving statistics 2e-5 + 2e-5 |ref|, losses 1e-5 relative).  From four
blocks on the project had no bound: there the result must be within max(that bound, 4 x the error of
the float32 oracle against the float64 oracle on the same case), measured on the CPU inside the test
-- the kernels split K over up to 16 waves and combine the partials in another association than
numpy's pairwise sum.  The measured errors and bounds are printed (MEASUREMENTS.md, section 17)."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _p3d  # noqa: E402
import exact_models  # noqa: E402
import linear_model  # noqa: E402
import predict_3dpose  # noqa: E402
import shape_cases as sc  # noqa: E402
from _p3d import ptr  # noqa: E402
from oracle import ref_eval, ref_mlp  # noqa: E402
from test_gpu_exact import _tags  # noqa: E402

CUS = torch.cuda.get_device_properties(0).multi_processor_count
NAMES = list(sc.LIFTER_SHAPES)
LR = 1e-3


def _model(cfg, st, max_batch=64, seed=exact_models.BACKWARD_SEED, batch=64):
    m = linear_model.LinearModel(cfg.linear_size, cfg.num_layers, cfg.residual, cfg.batch_norm, False, batch, LR,
                                 "/tmp/p3d_shapes", cfg.predict_14, seed=seed, max_batch=max(max_batch, 64))
    m.set_weights({**st.params, **st.moving})
    return m


def _random(name, seed=1, bn_seed=2, **kw):
    cfg = sc.lifter_cfg(name)
    st = ref_mlp.init_state(cfg, seed=seed, bn_seed=bn_seed)
    return cfg, st, _model(cfg, st, **kw)


def _deep(cfg):
    return cfg.num_layers >= 4


def _bounded(got, ref, ref32, atol, rtol, deep, what, quiet=False):
    """|got - ref| <= atol + rtol |ref|, the project's bound -- or, on a deep model, 4 x the float32
    oracle's own error where that is larger.  Prints the measured error and the bound."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    tol = atol + rtol * np.abs(ref)
    e32 = float(np.abs(np.asarray(ref32, np.float64) - ref).max()) if deep else 0.0
    if deep:
        tol = np.maximum(tol, 4.0 * e32)
    err = np.abs(got - ref)
    if not quiet:
        print("%s: gpu err %.3g, float32-oracle err %.3g, bound %.3g" % (what, err.max(), e32, float(np.max(tol))))
    assert np.all(err <= tol), "%s: err %.3g (%.3g over its bound)" % (what, float(err.max()), float((err - tol).max()))


# ---- inference, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_forward_bit_exact_with_the_expected_launches(name):
    """forward_device on the integer model at B = 1, 4 (k_gemv: chain, fold or plain launches), 5, 37,
    64 (per-layer k_fwd), 65 and 300 (k_gemm_f32 from 256 rows where L % 128 == 0): the oracle's bits
    and the expected tags; once more from workspace row 16."""
    batches = sc.forward_batches(name)
    cfg, st = sc.lifter_exact_case(name, batches[0])[:2]
    m = _model(cfg, st, max_batch=max(batches) + 16)
    for B in batches:
        _, _, x, ref = sc.lifter_exact_case(name, B)
        xd = torch.from_numpy(np.array(x)).cuda()
        out = {}
        tags = _tags(m, lambda: out.update(y=m.forward_device(xd)))
        np.testing.assert_array_equal(out["y"].cpu().numpy(), ref, err_msg="%s B=%d" % (name, B))
        assert tags == sc.expected_forward_tags(cfg, B, CUS), (name, B, tags)
        m.check_errors()
    for B in (batches[1], batches[-1] if batches[-1] <= 64 else 37):    # a k_gemv form and a k_fwd chain
        _, _, x, ref = sc.lifter_exact_case(name, B)
        y = m.forward_device(torch.from_numpy(np.array(x)).cuda(), ws_row=16)
        np.testing.assert_array_equal(y.cpu().numpy(), ref, err_msg="%s B=%d ws_row 16" % (name, B))
    m.check_errors()
    m.close()


# ---- serve ----------------------------------------------------------------------------------------------
def _pcfg(cfg, max_batch=64):
    return _p3d.P3DCfg(cfg.linear_size, cfg.num_layers, int(cfg.residual), int(cfg.batch_norm), 0, 32, 48,
                       _p3d.P3D_DTYPE_F32, max_batch, 1e-3, 0.99)


@pytest.mark.parametrize("name", [n for n in NAMES if sc.serve_expected(sc.lifter_cfg(n), 64) == "runs"])
def test_serve_bit_exact_on_the_planned_kernel(name):
    """p3d_serve at one request, 20 requests + 5 rows and 33 requests + 1 row (a long launch) == the
    exact forward; the kernel it launched is the one p3d_serve_plan names."""
    cfg, st = sc.lifter_exact_case(name, 64)[:2]
    m = _model(cfg, st)
    lib = _p3d.lib()
    pcfg = _pcfg(cfg)
    for B in sc.SERVE_BATCHES:
        _, _, x, ref = sc.lifter_exact_case(name, B)
        y = m.serve_device(torch.from_numpy(np.array(x)).cuda())
        torch.cuda.synchronize()
        m.serve_check()
        np.testing.assert_array_equal(y.cpu().numpy(), ref, err_msg="%s B=%d" % (name, B))
        ran, planned = ctypes.create_string_buffer(128), ctypes.create_string_buffer(128)
        _p3d.check(lib.p3d_kernel_name(m._h, 3, ran, 128), "p3d_kernel_name")
        _p3d.check(lib.p3d_serve_plan(ctypes.byref(pcfg), CUS, B, 0, planned, 128, None), "p3d_serve_plan")
        assert ran.value == planned.value, (name, B, ran.value, planned.value)
        print(name, B, ran.value.decode())
    m.check_errors()
    m.close()


@pytest.mark.parametrize("name", [n for n in NAMES if sc.serve_expected(sc.lifter_cfg(n), 64) == "refused"])
def test_serve_refusal_and_the_drivers_fall_back(name):
    """A shape p3d_serve does not take: the call returns P3D_ERR_ARG with the documented message and
    leaves serve_check clean; LinearModel.step(isTraining=False) takes the cached-graph path and
    returns the exact forward and the oracle's loss; predict_3dpose.evaluate_batches (up to three
    blocks, random weights) equals the oracle's evaluation."""
    cfg, st, x, ref = sc.lifter_exact_case(name, 64)
    m = _model(cfg, st)
    xd = torch.from_numpy(np.array(x)).cuda()
    y = torch.full((64, 48), 7.0, device="cuda")
    assert _p3d.lib().p3d_serve(m._h, ptr(xd), 64, ptr(y), m.stream()) == _p3d.P3D_ERR_ARG
    assert _p3d.lib().p3d_last_error().decode() == sc.SERVE_REFUSAL
    torch.cuda.synchronize()
    m.serve_check()
    assert bool((y == 7.0).all())
    t = exact_models.integer_inputs(64, seed=11, dim=48)
    for _ in range(2):
        loss, _, out = m.step(None, np.array(x), t, 1.0, isTraining=False)
    assert m._serve_steps.get(64) is None
    np.testing.assert_array_equal(out, ref)
    rl, _ = ref_mlp.eval_step(st, x, t)
    assert abs(loss - rl) <= 1e-5 * max(1.0, abs(rl)), (loss, rl)
    m.check_errors()
    m.close()
    if cfg.num_layers > 3:
        return
    cfg, st, m = _random(name, seed=3, bn_seed=4)
    stats = ref_eval.synthetic_stats()
    rng = np.random.default_rng(17)
    enc = [rng.standard_normal((64, 32)) for _ in range(3)]
    dec = [rng.standard_normal((64, 48)) for _ in range(3)]
    err, jerr, _, loss = predict_3dpose.evaluate_batches(
        None, m, stats["mean3"], stats["std3"], stats["use3"], stats["ign3"], stats["mean2"], stats["std2"],
        stats["use2"], stats["ign2"], 0, enc, dec)
    r_err, r_jerr, r_loss = ref_eval.evaluate_batches(lambda e, d: ref_mlp.eval_step(st, e, d), enc, dec,
                                                      stats["mean3"], stats["std3"], stats["use3"], stats["ign3"])
    print(name, "MPJPE |d| %.3g mm, loss rel %.3g" % (abs(err - r_err), abs(loss - r_loss) / max(1, r_loss)))
    assert abs(err - r_err) <= 1e-4, (err, r_err)
    np.testing.assert_allclose(jerr, r_jerr, atol=1e-4)
    assert abs(loss - r_loss) <= 1e-5 * max(1, r_loss)
    m.close()


# ---- inference against the float64 oracle -------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_forward_random_weights_vs_oracle(name):
    """Random weights at B = 37 and 300 against the float64 oracle: 5e-5 + 5e-5 |ref| up to three
    blocks, beyond that max(it, 4 x the float32 oracle's error)."""
    cfg, st, m = _random(name, max_batch=300)
    for B in sc.ORACLE_BATCHES:
        x = np.random.default_rng(B).standard_normal((B, 32)).astype(np.float32)
        y = m.forward_device(torch.from_numpy(x).cuda()).cpu().numpy()
        ref, _ = ref_mlp.forward(st, x, False)
        ref32 = ref_mlp.forward(st, x, False, dt=np.float32)[0] if _deep(cfg) else None
        _bounded(y, ref, ref32, 5e-5, 5e-5, _deep(cfg), "%s B=%d forward" % (name, B))
    m.check_errors()
    m.close()


# ---- training, bit for bit ------------------------------------------------------------------------------
def _exact_step(m, case, poison):
    """One training forward + p3d_backward of a lifter_backward_case on model m (the pattern of
    tests/test_gpu_exact.py): outputs, every gradient and the untouched dy by assert_array_equal;
    returns the backward's tags.  poison: over a NaN-filled gradient buffer."""
    cfg, st, x, dy, keep, row0, out, grads = case
    B = dy.shape[0]
    xd = torch.tensor(x).cuda()
    dyd = torch.tensor(dy).cuda()
    assert dyd.data_ptr() % 16 == 0
    if poison:
        m.flat["grads"].fill_(float("nan"))
    y = m.forward_device(xd, True, keep, ctr=exact_models.BACKWARD_CTR, row_offset=row0)
    np.testing.assert_array_equal(y.cpu().numpy(), out, err_msg="training forward")
    tags = _tags(m, lambda: _p3d.check(_p3d.lib().p3d_backward(m._h, ptr(dyd), B, m.stream()), "p3d_backward"))
    torch.cuda.synchronize()
    assert sorted(m.trainable_names()) == sorted(grads)
    for n in m.trainable_names():
        np.testing.assert_array_equal(m.grad(n).cpu().numpy(), grads[n], err_msg=n)
    np.testing.assert_array_equal(dyd.cpu().numpy(), dy, err_msg="dy was written")
    m.check_errors()
    return tags


@pytest.mark.parametrize("name", sc.train_names())
def test_backward_bit_exact_with_the_expected_launches(name):
    """The training forward (dropout at keep 0.5) and p3d_backward on the entry's integer twin
    without BN == the oracle, bit for bit, at B = 17 and 64 (L64_N1 also at 256 and 257, L128_N3
    also from row offset 192), each twice on one model, the second time over NaN-filled gradients;
    the backward's tags are the expected ones (one k_wgrad_grad launch up to 16 layers, per-layer
    k_wgrad beyond)."""
    runs = [r for r in sc.backward_runs() if r[0] == name]
    cfg, st = sc.lifter_backward_case(*runs[0])[:2]
    m = _model(cfg, st, max_batch=max(r[1] for r in runs))
    for run in runs:
        case = sc.lifter_backward_case(*run)
        want = sc.expected_backward_tags(cfg, run[1], CUS)
        for poison in (False, True):
            got = _exact_step(m, case, poison)
            assert got == want, (run, got)
    m.close()


# ---- training with BN against the float64 oracle ------------------------------------------------------
def _pre_bn_bias(name):
    return "/b1" in name or "/b2_" in name or "/b3_" in name


@pytest.mark.parametrize("name,B", sc.bn_runs())
def test_bn_gradients_vs_oracle(name, B):
    """p3d_train_fwd_bwd (keep 0.5; the output layer with the fused MSE at L64_N0, as k_out_part
    elsewhere up to 256 rows) against the float64 oracle in the pattern of test_gpu_parity's
    _grad_check: loss, y, every gradient, the moving statistics; the step's tags."""
    cfg = sc.lifter_cfg(name, batch_norm=True)
    deep = _deep(cfg)
    st = ref_mlp.init_state(cfg, seed=1, bn_seed=2)
    m = _model(cfg, st, max_batch=B, seed=11, batch=B)
    rng = np.random.default_rng(9)
    x = rng.standard_normal((B, 32)).astype(np.float32)
    t = rng.standard_normal((B, 48)).astype(np.float32)
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    y = torch.empty((B, 48), device="cuda")
    tags = _tags(m, lambda: _p3d.check(_p3d.lib().p3d_train_fwd_bwd(
        m._h, ptr(xd), ptr(td), B, ptr(y), sc.TRAIN_KEEP, m.seed, 0, ptr(m._loss_dev), m.stream()), "p3d_train_fwd_bwd"))
    torch.cuda.synchronize()
    want = dict(sc.expected_forward_tags(cfg, B, CUS, training="step"))
    for k, v in sc.expected_backward_tags(cfg, B, CUS).items():
        want[k] = want.get(k, 0) + v
    assert tags == want, (name, B, tags)
    assert ("fwd_out_train" in tags) == (name == "L64_N0" or B > 256) and ("fwd_out_part" in tags) != ("fwd_out_train" in tags)
    res = {}
    for dt in ((np.float64, np.float32) if deep else (np.float64,)):
        out, cache = ref_mlp.forward(st, x, True, sc.TRAIN_KEEP, m.seed, 0, 0, dt=dt)
        rl, dy = ref_mlp.mse(out, t, dt)
        st2 = st.copy()
        ref_mlp.bn_update(st2, cache, dt)
        res[dt] = (out, float(rl), ref_mlp.backward(st, cache, dy, dt), st2.moving)
    out, rl, grads, moving = res[np.float64]
    r32 = res.get(np.float32)
    _bounded(y.cpu().numpy(), out, r32[0] if deep else None, 5e-5, 5e-5, deep, "%s B=%d y" % (name, B))
    ltol = 1e-5 * max(1.0, rl)
    if deep:
        ltol = max(ltol, 4 * abs(r32[1] - rl))
    loss = float(m._loss_dev.item())
    print("%s B=%d loss: gpu err %.3g, bound %.3g" % (name, B, abs(loss - rl), ltol))
    assert abs(loss - rl) <= ltol
    worst = (0.0, 0.0, "")
    for n in m.trainable_names():
        g, r = m.grad(n).cpu().numpy(), grads[n]
        if _pre_bn_bias(n):            # analytically zero under BN: noise-sized
            assert np.abs(g).max() < 1e-4, n
            continue
        scale = max(np.abs(r).max(), 1e-30)
        tol = 1e-3 * scale
        if deep:
            tol = max(tol, 4 * float(np.abs(r32[2][n] - r).max()))
        err = float(np.abs(g - r).max())
        worst = max(worst, (err / tol, err / scale, n))
        assert err <= tol, "%s: err %.3g over %.3g" % (n, err, tol)
    print("%s B=%d gradients: worst err / bound %.3g (rel %.3g, %s)" % ((name, B) + worst))
    for k, v in moving.items():
        _bounded(m.variable(k).cpu().numpy(), v, r32[3][k] if deep else None, 2e-5, 2e-5, deep, k, quiet=True)
    m.check_errors()
    m.close()


# ---- steps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L64_N0", "L192_N2", "L128_N8"])
def test_three_train_steps_track_the_oracle(name):
    """Three LinearModel.step(isTraining=True) calls against ref_mlp's TF1 Adam oracle at the bounds
    of test_train_steps_track_oracle (loss 1e-5 relative, outputs 1e-4, weights 5e-5; pre-BN biases
    within Adam's step bound) -- at eight blocks max(those, 4 x the float32 oracle's error)."""
    cfg, st, m = _random(name, seed=11)
    deep = _deep(cfg)
    st32 = st.copy()
    init = {k: np.array(v, copy=True) for k, v in st.params.items()}
    rng = np.random.default_rng(21)
    for step in range(3):
        x, t = rng.standard_normal((64, 32)), rng.standard_normal((64, 48))
        loss, _, _, out = m.step(None, x, t, 0.5, isTraining=True)
        rl, ro = ref_mlp.train_step(st, x, t, 0.5, LR, seed=m.seed, ctr=step)
        r32 = ref_mlp.train_step(st32, x, t, 0.5, LR, seed=m.seed, ctr=step, dt=np.float32) if deep else None
        ltol = 1e-5 * max(1.0, rl)
        if deep:
            ltol = max(ltol, 4 * abs(float(r32[0]) - rl))
        print("%s step %d loss: gpu err %.3g, bound %.3g" % (name, step, abs(loss - rl), ltol))
        assert abs(loss - rl) <= ltol, (step, loss, rl)
        _bounded(out, ro, r32[1] if deep else None, 1e-4, 1e-4, deep, "%s step %d outputs" % (name, step))
    gs, b1, b2 = m.get_step()
    assert gs == 3 and abs(b1 - 0.9 ** 4) < 1e-6 and abs(b2 - 0.999 ** 4) < 1e-6
    w = m.get_weights()
    for n in m.trainable_names():
        if cfg.batch_norm and _pre_bn_bias(n):
            # Adam's step bound over 3 steps (test_train_steps_track_oracle's argument): 3 x 1.85 lr
            assert np.abs(w[n] - init[n]).max() <= 3 * 1.85 * LR * 1.001, n
            continue
        tol = 5e-5
        if deep:
            tol = max(tol, 4 * float(np.abs(st32.params[n].astype(np.float64) - st.params[n]).max()))
        err = float(np.abs(w[n] - st.params[n]).max())
        assert err < tol, (n, err, tol)
    m.check_errors()
    m.close()


@pytest.mark.parametrize("name", ["L128_N8", "L64_N0"])
def test_fused_train_step_bit_identical_to_unfused(name):
    """p3d_train_step (Adam inside the weight-gradient kernels; at 18 layers the per-layer k_wgrad
    and no fused tail, so the step state advances in a launch of its own) == p3d_train_fwd_bwd_lr +
    p3d_adam_apply over three steps: outputs, loss, weights, slots, moving statistics, step."""
    cfg = sc.lifter_cfg(name)
    st = ref_mlp.init_state(cfg, seed=4, bn_seed=5)
    fused, plain = _model(cfg, st, seed=9), _model(cfg, st, seed=9)
    lib = _p3d.lib()
    rng = np.random.default_rng(3)
    for step in range(3):
        x = torch.from_numpy(rng.standard_normal((64, 32)).astype(np.float32)).cuda()
        t = torch.from_numpy(rng.standard_normal((64, 48)).astype(np.float32)).cuda()
        yf, yp = torch.empty((64, 48), device="cuda"), torch.empty((64, 48), device="cuda")
        tags = _tags(fused, lambda: fused.train_step_device(x, t, 0.5, out=yf))
        _p3d.check(lib.p3d_train_fwd_bwd_lr(plain._h, ptr(x), ptr(t), 64, ptr(yp), 0.5, plain.seed, 0, plain.lr0,
                                            100000.0, 0.96, ptr(plain._loss_dev), plain.stream()), "p3d_train_fwd_bwd_lr")
        _p3d.check(lib.p3d_adam_apply(plain._h, plain.stream()), "p3d_adam_apply")
        assert torch.equal(yf, yp), step
        assert torch.equal(fused._loss_dev, plain._loss_dev), step
        want = dict(sc.expected_forward_tags(cfg, 64, CUS, training="step"))
        want.update(sc.expected_backward_tags(cfg, 64, CUS))
        assert tags == want, (name, step, tags)
    for k in ("params", "moving", "adam_m", "adam_v"):
        if fused.flat[k] is not None:
            assert torch.equal(fused.flat[k], plain.flat[k]), k
    assert fused.get_step() == plain.get_step() and fused.get_step()[0] == 3
    x = torch.from_numpy(rng.standard_normal((64, 32)).astype(np.float32)).cuda()
    assert torch.equal(fused.forward_device(x), plain.forward_device(x))
    for m in (fused, plain):
        m.check_errors()
        m.close()


def test_per_layer_wgrad_reads_the_dy_of_its_own_step(monkeypatch):
    """The per-layer k_wgrad form (P3D_WGRAD_MULTI=0, as every model above 16 layers takes it) behind
    k_out_part: dy is formed by the output layer's data-gradient launch, so that layer's weight
    gradient must follow it.  Two p3d_train_fwd_bwd calls on different batches at L64_N1, each
    gradient of w4 / b4 against the float64 oracle (launched ahead, k_wgrad read the previous
    call's dy -- zeros in the first)."""
    monkeypatch.setenv("P3D_WGRAD_MULTI", "0")
    cfg = sc.lifter_cfg("L64_N1")
    st = ref_mlp.init_state(cfg, seed=1, bn_seed=2)
    m = _model(cfg, st, seed=11)
    rng = np.random.default_rng(31)
    for call in range(2):
        x = rng.standard_normal((64, 32)).astype(np.float32)
        t = rng.standard_normal((64, 48)).astype(np.float32)
        xd, td, y = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda(), torch.empty((64, 48), device="cuda")
        tags = _tags(m, lambda: _p3d.check(_p3d.lib().p3d_train_fwd_bwd(
            m._h, ptr(xd), ptr(td), 64, ptr(y), 1.0, m.seed, 0, ptr(m._loss_dev), m.stream()), "p3d_train_fwd_bwd"))
        torch.cuda.synchronize()
        assert tags.get("fwd_out_part") == 1 and tags.get("wgrad") == 4 and "wgrad_multi" not in tags, tags
        out, cache = ref_mlp.forward(st, x, True, 1.0, m.seed, 0, 0)
        grads = ref_mlp.backward(st, cache, ref_mlp.mse(out, t)[1])
        for n in ("linear_model/w4", "linear_model/b4", "linear_model/w1"):
            g, r = m.grad(n).cpu().numpy(), grads[n]
            assert np.abs(g - r).max() <= 1e-3 * np.abs(r).max(), (call, n)
        # (BN's moving statistics moved with the call: the oracle's state follows)
        ref_mlp.bn_update(st, cache)
    m.check_errors()
    m.close()
