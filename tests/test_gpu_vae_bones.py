"""GPU tests of the bones filter (the bones kind of csrc/p3d_vae.h, csrc/p3d_bones.h,
models.VAEBones, models.Pose3DVaeBones, losses.loss_bones, top_vae_3d_pose/bones.py and the
pose_3d_bones.py driver) against tests/vae_bones_oracle.py and the reference's own conversions
(tests/golden/bones_goldens.npz).

Bounds are the project's (tests/test_gpu_vae_wide.py): forward values and row terms 2e-5 + 2e-5 |ref|
vs the float64 oracle, loss vectors 1e-5 relative, gradients 1e-3 of each tensor's largest entry,
integer models bit for bit (tests/vae_bones_exact.py proves them exact), five teacher-forced
training steps 5e-5 on the weights, the conversions bit for bit.
"""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import vae_bones_exact as vx
import vae_bones_oracle as vb
from top_vae_3d_pose import bones, models

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = {
    "wide1376": (1376, (40, 32), 24, (32, 40)),     # [x2d | mag | cos | effnet_out]
    "narrow64": (64, (40, 32), 24, (32, 40)),       # bones alone: one launch per step
    "edge": (264, (8,), 8, (8,)),                   # mag1 has K = 8 (the padded k tile); the first width past the LDS form
}
BATCHES = (1, 17, 64, 65, 200)          # 17: one row past the 16-row round; 65: one row past the 64-row block
GRAD_BATCHES = (17, 64, 65, 200)
FACTORS = (10.0, 100.0, 1.0, 100.0)     # train.yml's mag, cos, dkl, ang
LR = 1e-3


def rand_params(shape, seed):
    P = vb.init_params(shape, seed)
    rng = np.random.default_rng(seed + 1)
    for k in P:
        if k.endswith("/bias"):
            P[k] = (0.1 * rng.standard_normal(P[k].shape)).astype(np.float32)
    return P


_models, _cases = {}, {}


def model_of(name):
    if name not in _models:
        shape = SHAPES[name]
        m = models.VAEBones(shape[0], shape[2], shape[1], shape[3], max_batch=256, seed=5)
        m.set_weights(rand_params(shape, 3))
        _models[name] = m
    return _models[name]


def case_of(name, B):
    """Inputs and the float64 oracle's forward / loss / backward at (shape, B), computed once."""
    if (name, B) not in _cases:
        shape = SHAPES[name]
        rng = np.random.default_rng(100 * B + len(name))
        x = rng.standard_normal((B, shape[0])).astype(np.float32)
        t = rng.standard_normal((B, 64)).astype(np.float32)
        eps = rng.standard_normal((B, shape[2])).astype(np.float32)
        P = rand_params(shape, 3)
        c = vb.forward(P, shape, x, eps)
        terms = vb.row_terms(c, t)
        g, _ = vb.backward(P, shape, c, t, FACTORS)
        _cases[(name, B)] = dict(x=x, t=t, eps=eps, c=c, terms=terms, loss=vb.loss4(terms, FACTORS), g=g)
    return _cases[(name, B)]


def close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref) - (2e-5 + 2e-5 * np.abs(ref))
    print(what, "max |err| %.3g" % float(np.abs(got - ref).max()))
    assert err.max() <= 0, (what, float(np.abs(got - ref).max()))


def same_bits(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=what)
    view = np.uint32 if got.dtype == np.float32 else np.uint64
    ok = np.isnan(ref) | (got.view(view) == ref.view(view))
    assert ok.all(), (what, int((~ok).sum()))


def test_param_table_kind_and_refusals():
    import _p3d
    m = model_of("wide1376")
    assert [(n, s) for n, s, _ in m.param_table] == vb.param_names(SHAPES["wide1376"])
    assert _p3d.lib().p3d_vae_kind(m._h) == 1 and m.output_size == 64
    n = model_of("narrow64")
    assert [(nm, s) for nm, s, _ in n.param_table] == vb.param_names(SHAPES["narrow64"])
    plain = models.VAE(48, 24, [40, 32], [32, 40], max_batch=16, seed=1, init=False)
    assert _p3d.lib().p3d_vae_kind(plain._h) == 0
    plain.close()
    for mm in (m, n):        # (narrow64: in == out, which a joint filter would serve as seq_len 1)
        with pytest.raises(ValueError):
            mm.filter_sequences(torch.zeros((4, 64), device="cuda"), [0, 4])
    dev = torch.zeros((4, 64), device="cuda")
    off = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    rc = _p3d.lib().p3d_vae_seq_filter(n._h, _p3d.ptr(dev), _p3d.ptr(off), 1, 4, None, 0, 0, None, None, None,
                                       _p3d.ptr(dev), None, None, None)
    assert rc == _p3d.P3D_ERR_ARG
    with pytest.raises(ValueError):
        m.loss_device(np.zeros((4, 1376), np.float32), np.zeros((4, 64), np.float32), (1.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        m.loss_device(np.zeros((4, 1376), np.float32), np.zeros((4, 48), np.float32), FACTORS)
    with pytest.raises(ValueError):
        models.VAEBones(1376, 24, [40, 32], [32, 40], human_3d_size=42)
    with pytest.raises(ValueError):
        models.VAEBones(1370, 24, [40, 32], [32, 40])


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_vs_oracle(name, B):
    m, k = model_of(name), case_of(name, B)
    o = m.forward_device(k["x"], eps=k["eps"], target=k["t"], want=("y", "mean", "log_var", "z"))
    for key in ("y", "mean", "log_var", "z"):
        close(o[key].cpu().numpy(), k["c"][key], key)
    assert tuple(o["row_terms"].shape) == (B, 4)
    close(o["row_terms"].cpu().numpy(), k["terms"], "row_terms")
    loss = m.loss_device(k["x"], k["t"], FACTORS, eps=k["eps"]).cpu().numpy()
    assert loss.shape == (4,)
    np.testing.assert_allclose(loss, k["loss"], rtol=1e-5, atol=0)
    mag, cos = m(k["x"], eps=k["eps"])
    assert torch.equal(mag, o["y"][:, :16]) and torch.equal(cos, o["y"][:, 16:])


@pytest.mark.parametrize("B", GRAD_BATCHES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_gradients_vs_oracle(name, B):
    m, k = model_of(name), case_of(name, B)
    loss = m.compute_gradients(k["x"], k["t"], FACTORS, eps=k["eps"]).cpu().numpy()
    np.testing.assert_allclose(loss, k["loss"], rtol=1e-5, atol=0)
    g = m.grads()
    assert sorted(g) == sorted(k["g"])
    for n, ref in k["g"].items():
        err = float(np.abs(g[n] - ref).max())
        print("grad", name, B, n, "err %.3g of max %.3g" % (err, np.abs(ref).max()))
        assert err <= 1e-3 * np.abs(ref).max(), (n, err, float(np.abs(ref).max()))


@pytest.mark.parametrize("B", (16, 64, 128))
@pytest.mark.parametrize("name", ("wide1376", "narrow64"))
def test_integer_model_bit_exact(name, B):
    """y, mean, z, the ANG row terms and every gradient of the integer model equal the oracle bit for
    bit, in forms 0 and 1 where B <= 64, the second run of each over a NaN-filled gradient buffer
    and workspace."""
    shape = SHAPES[name]
    k = vx.exact_case(B, shape)
    m = models.VAEBones(shape[0], shape[2], shape[1], shape[3], max_batch=B, seed=1)
    m.set_weights(k["P"])
    o = m.forward_device(k["x"], eps=k["eps"], target=k["t"], want=("y", "mean", "z"))
    for key in ("y", "mean", "z"):
        np.testing.assert_array_equal(o[key].cpu().numpy(), k[key], err_msg=key)
    np.testing.assert_array_equal(o["row_terms"][:, 3].cpu().numpy(), k["ang"])
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
    m = models.VAEBones(shape[0], shape[2], shape[1], shape[3], max_batch=max_batch, seed=1)
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


@pytest.mark.parametrize("widths,table_rows", (((32, 64, 1280), 300), ((32, 64), 0)), ids=("wide1376", "narrow96"))
def test_cat_equals_the_materialised_input(widths, table_rows):
    """Segments -- the wide one a (table, idx) pair whose index repeats rows and leaves the table once
    on each side -- give the bits of the plain call on torch.cat of the gathered rows: y, the loss
    vector, every gradient, and after three training steps the weights and both Adam slots."""
    n_in = sum(widths)
    shape = (n_in, (40, 32), 24, (32, 40))
    B = 70
    rng = np.random.default_rng(9)
    dev = torch.device("cuda")
    segs, mat = [], []
    for w in widths:
        if w == 1280:
            table = torch.from_numpy(rng.standard_normal((table_rows, w)).astype(np.float32)).to(dev)
            idx = rng.integers(0, table_rows, size=B)
            idx[3] = idx[2]
            idx[10], idx[11] = -5, table_rows + 7
            idx = torch.from_numpy(idx.astype(np.int64)).to(dev)
            segs.append((table, idx))
            mat.append(table[idx.clamp(0, table_rows - 1)])
        else:
            segs.append(torch.from_numpy(rng.standard_normal((B, w)).astype(np.float32)).to(dev))
            mat.append(segs[-1])
    x = torch.cat(mat, dim=1).contiguous()
    t = torch.from_numpy(rng.standard_normal((B, 64)).astype(np.float32)).to(dev)
    eps = torch.from_numpy(rng.standard_normal((B, 24)).astype(np.float32)).to(dev)
    P = rand_params(shape, 4)
    a, b = _fresh(shape, P, max_batch=128), _fresh(shape, P, max_batch=128)
    ya = a.forward_device(segs, eps=eps, target=t)
    yb = b.forward_device(x, eps=eps, target=t)
    assert torch.equal(ya["y"], yb["y"]) and bool(torch.isfinite(ya["y"]).all())
    assert torch.equal(ya["row_terms"], yb["row_terms"])
    la = a.loss_device(segs, t, FACTORS, eps=eps).clone()
    assert torch.equal(la, b.loss_device(x, t, FACTORS, eps=eps))
    la = a.compute_gradients(segs, t, FACTORS, eps=eps).clone()
    assert torch.equal(la, b.compute_gradients(x, t, FACTORS, eps=eps))
    assert torch.equal(a.flat("grads"), b.flat("grads")) and bool(a.flat("grads").abs().sum() > 0)
    for _ in range(3):
        la = a.train_step_device(segs, t, FACTORS, LR, eps=eps).clone()
        assert torch.equal(la, b.train_step_device(x, t, FACTORS, LR, eps=eps))
    for which in ("params", "adam_m", "adam_v"):
        assert torch.equal(a.flat(which), b.flat(which)), which
    assert a.get_step()[0] == b.get_step()[0] == 3
    a.close()
    b.close()


@pytest.mark.parametrize("name", ("wide1376", "narrow64"))
def test_forms_agree_and_graph_replays(name):
    """B = 64 over 4 steps: train_step == grad + adam_apply == form 1 == a captured graph of the 4
    steps on one stream, bit for bit."""
    shape = SHAPES[name]
    P = rand_params(shape, 8)
    rng = np.random.default_rng(77)
    xs = torch.from_numpy(rng.standard_normal((4, 64, shape[0])).astype(np.float32)).cuda()
    ts = torch.from_numpy(rng.standard_normal((4, 64, 64)).astype(np.float32)).cuda()
    es = torch.from_numpy(rng.standard_normal((4, 64, 24)).astype(np.float32)).cuda()
    one, two, part, graph = _fresh(shape, P), _fresh(shape, P), _fresh(shape, P, form=1), _fresh(shape, P)
    losses = []
    for s in range(4):
        losses.append(one.train_step_device(xs[s], ts[s], FACTORS, LR, eps=es[s]).cpu().numpy().copy())
        two.compute_gradients(xs[s], ts[s], FACTORS, eps=es[s])
        two.adam_apply(LR)
        lp = part.train_step_device(xs[s], ts[s], FACTORS, LR, eps=es[s]).cpu().numpy()
        np.testing.assert_array_equal(lp, losses[-1])
    torch.cuda.synchronize()
    assert one.get_step()[0] == two.get_step()[0] == part.get_step()[0] == 4
    ref = _state(one)
    _same(_state(two), ref, "grad + adam_apply")
    _same(_state(part), ref, "partials form")
    assert all(np.abs(ref[0][n] - P[n]).max() > 0 for n in P)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    lg = torch.zeros((4, 4), device="cuda")
    with torch.cuda.stream(side):
        graph.train_step_device(xs[0], ts[0], FACTORS, LR, eps=es[0], loss_out=lg[0])
    torch.cuda.synchronize()
    graph.set_weights(P)
    graph.flat("adam_m").zero_()
    graph.flat("adam_v").zero_()
    graph.set_step(0, 0.9, 0.999)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for s in range(4):
            graph.train_step_device(xs[s], ts[s], FACTORS, LR, eps=es[s], loss_out=lg[s])
    g.replay()
    torch.cuda.synchronize()
    assert graph.get_step()[0] == 4
    _same(_state(graph), ref, "graph")
    np.testing.assert_array_equal(lg.cpu().numpy(), np.stack(losses))
    for m in (one, two, part, graph):
        m.close()


def test_five_steps_track_the_oracles_adam():
    """Five teacher-forced training steps at shape wide1376: from the device's own state before each
    step, the float64 oracle's whole step lands within 5e-5 of the device's new weights."""
    import vae_oracle as vo
    shape = SHAPES["wide1376"]
    P = rand_params(shape, 12)
    m = _fresh(shape, P)
    rng = np.random.default_rng(5)
    f64, f32 = np.float64, np.float32
    for step in range(5):
        x = rng.standard_normal((64, shape[0])).astype(f32)
        t = rng.standard_normal((64, 64)).astype(f32)
        eps = rng.standard_normal((64, 24)).astype(f32)
        w0, m0, v0 = _state(m)
        assert m.get_step()[0] == step
        m.train_step_device(x, t, FACTORS, LR, eps=eps)
        torch.cuda.synchronize()
        w1, _, _ = _state(m)
        gref, _ = vb.backward(w0, shape, vb.forward(w0, shape, x, eps), t, FACTORS)
        worst = 0.0
        for n in w0:
            wo, _, _ = vo.adam_apply(w0[n].astype(f64), m0[n].astype(f64), v0[n].astype(f64), gref[n], LR, step + 1)
            err = float(np.abs(w1[n] - wo).max())
            worst = max(worst, err)
            assert err < 5e-5, (step, n, err)
        print("step", step, "worst weight error %.3g" % worst)
    m.close()


def _goldens():
    with np.load(os.path.join(HERE, "golden", "bones_goldens.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("N", (1, 63, 64, 65))
def test_conversions_match_the_reference_bit_for_bit(N):
    """p3d_bones_from_joints(precise=1) and p3d_bones_to_joints against the reference's own outputs
    (rows tiled past 64 where N asks), NaNs in the same places; precise=0 against the float32 oracle."""
    g = _goldens()
    rows = (np.arange(N) + (62 if N == 1 else 0)) % 64        # (N = 1: the row with the zero-length bone)
    j = g["joints"][rows]
    b = bones.convert_to_bones(j).cpu().numpy()
    same_bits(b[:, :16], g["mag"][rows], "mag")
    same_bits(b[:, 16:], g["cos"][rows], "cos")
    b32 = bones.convert_to_bones(torch.from_numpy(j).cuda(), precise=False).cpu().numpy()
    same_bits(b32, vb.bones_from_joints(j, np.float32), "float32 bones")
    both = torch.from_numpy(np.concatenate([g["mag"], g["cos"]], axis=1)[rows]).cuda()
    same_bits(bones.convert_to_joints(both).cpu().numpy(), g["back"][rows], "back")
    free = np.concatenate([g["free_mag"], g["free_cos"]], axis=1)[rows]
    same_bits(bones.convert_to_joints(free).cpu().numpy(), g["free_back"][rows], "free_back")
    same_bits(bones.convert_to_joints(g["free_mag"][rows], g["free_cos"][rows]).cpu().numpy(), g["free_back"][rows],
              "free_back (pair)")
    with pytest.raises(ValueError):
        bones.convert_to_bones(j[:, :40])
    with pytest.raises(ValueError):
        bones.convert_to_joints(free, bones_joints=(np.array(bones.BJB), np.array(bones.BJA)))


def test_conversion_is_capturable():
    g = _goldens()
    j = torch.from_numpy(g["joints"]).cuda()
    out = torch.zeros((64, 64), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bones.convert_to_bones(j, out=out)
    torch.cuda.synchronize()
    out.zero_()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=side):
        bones.convert_to_bones(j, out=out)
    gr.replay()
    torch.cuda.synchronize()
    same_bits(out.cpu().numpy(), np.concatenate([g["mag"], g["cos"]], axis=1), "captured")


@pytest.mark.parametrize("name", ("wide1376", "narrow64"))
def test_a_nan_row_stays_in_its_row_and_reaches_the_loss(name):
    m, k = model_of(name), case_of(name, 65)
    x = k["x"].copy()
    x[20, 5] = np.nan
    o = m.forward_device(x, eps=k["eps"], target=k["t"], want=("y", "mean", "z"))
    for key in ("y", "mean", "z", "row_terms"):
        got = o[key].cpu().numpy()
        assert np.isnan(got[20]).all(), key
        assert np.isfinite(np.delete(got, 20, axis=0)).all(), key
    clean = m.forward_device(k["x"], eps=k["eps"], target=k["t"], want=("y",))
    keep = [r for r in range(65) if r != 20]
    assert torch.equal(o["y"][keep], clean["y"][keep]) and torch.equal(o["row_terms"][keep], clean["row_terms"][keep])
    loss = m.loss_device(x, k["t"], FACTORS, eps=k["eps"]).cpu().numpy()
    assert np.isnan(loss).all()
    t = k["t"].copy()
    t[64, 16 + 4] = np.nan                      # a NaN target cosine (a zero-length bone): COS and ANG only
    o = m.forward_device(k["x"], eps=k["eps"], target=t, want=("y",))
    rt = o["row_terms"].cpu().numpy()
    assert np.isnan(rt[64, [1, 3]]).all() and np.isfinite(rt[64, [0, 2]]).all() and np.isfinite(rt[:64]).all()
    loss = m.loss_device(k["x"], t, FACTORS, eps=k["eps"]).cpu().numpy()
    assert np.isnan(loss[[1, 3]]).all() and np.isfinite(loss[[0, 2]]).all()
    m.compute_gradients(k["x"], t, FACTORS, eps=k["eps"])
    assert np.isnan(m.grads()["cos2/bias"]).any()


def test_pose3dvaebones_equals_the_oracles_composition():
    """Lifter (128 x 1) then the 1376-input bones filter on the device: out_3d against the lifter's
    oracle, (mag, cos) against the filter's oracle applied to [x, precise bones of the device's
    out_3d, features]; use_2d alone, bones alone, the float32 conversion, loss_bones, the argument
    errors."""
    import linear_model
    from oracle import ref_mlp
    from top_vae_3d_pose import args_def, losses
    cfg = ref_mlp.Cfg(linear_size=128, num_layers=1, residual=True, batch_norm=True)
    st = ref_mlp.init_state(cfg, seed=5, bn_seed=6)
    lifter = linear_model.LinearModel(128, 1, True, True, False, 64, 1e-3, "/tmp/p3d_vae_pose_bones", seed=7)
    lifter.set_weights({**st.params, **st.moving})
    pv = models.Pose3DVaeBones(24, [40, 32], [32, 40], use_effnet_ouptut=True, use_2d=True, pose3d=lifter,
                               max_batch=256, seed=3)
    shape = SHAPES["wide1376"]
    assert pv.vae.input_size == 1376 and pv.pred_bones and isinstance(pv.vae, models.VAEBones)
    P = rand_params(shape, 21)
    pv.vae.set_weights(P)
    rng = np.random.default_rng(2)
    x = rng.standard_normal((150, 32)).astype(np.float32)
    feat = (0.1 * rng.standard_normal((400, 1280))).astype(np.float32)
    idx = rng.permutation(400)[:150].astype(np.int64)
    eps = rng.standard_normal((150, 24)).astype(np.float32)
    F = torch.from_numpy(feat).cuda()
    xd = torch.from_numpy(x).cuda()
    out_3d, (mag, cos) = pv(xd, effnet_output=(F, torch.from_numpy(idx).cuda()), eps=eps)
    ref3d, _ = ref_mlp.forward(st, x, False, 1.0, 0, 0, 0)
    d = np.abs(out_3d.cpu().numpy() - ref3d)
    assert (d <= 5e-5 + 5e-5 * np.abs(ref3d)).all(), float(d.max())
    o3 = out_3d.cpu().numpy()
    b64 = vb.bones_from_joints(o3, np.float64)
    same_bits(bones.convert_to_bones(out_3d).cpu().numpy(), b64, "precise bones of out_3d")
    same_bits(pv.bones_tf(out_3d).cpu().numpy(), vb.bones_from_joints(o3, np.float32), "float32 bones of out_3d")
    xin = np.concatenate([x, b64, feat[idx]], axis=1)
    c = vb.forward(P, shape, xin, eps)
    close(mag.cpu().numpy(), c["mag"], "mag")
    close(cos.cpu().numpy(), c["cos"], "cos")
    _, (mag2, cos2) = pv(xd, effnet_output=torch.from_numpy(feat[idx]).cuda(), eps=eps)
    assert torch.equal(mag2, mag) and torch.equal(cos2, cos)
    # loss_bones under FLAGS' factors, the target a tensor or the reference's (mag, cos) pair
    t = rng.standard_normal((150, 64)).astype(np.float32)
    args_def.ENVIRON.setup(argv=["--mag_factor", "10", "--cos_factor", "100", "--ang_factor", "100"])
    try:
        lv = losses.loss_bones(pv.vae, torch.from_numpy(xin).cuda(), t, eps=eps).cpu().numpy()
        np.testing.assert_allclose(lv, vb.loss4(vb.row_terms(c, t), FACTORS), rtol=1e-5, atol=0)
        td = torch.from_numpy(t).cuda()
        lp = losses.loss_bones(pv.vae, torch.from_numpy(xin).cuda(), (td[:, :16], td[:, 16:]), eps=eps).cpu().numpy()
        np.testing.assert_array_equal(lp, lv)
    finally:
        args_def.ENVIRON.setup(argv=[])
    with pytest.raises(ValueError):
        pv(xd, effnet_output=F[:150, :1272].contiguous(), eps=eps)
    with pytest.raises(ValueError):
        pv(xd, effnet_output=F[:100], eps=eps)
    with pytest.raises(ValueError):
        pv(xd, eps=eps)
    with pytest.raises(ValueError):
        models.Pose3DVaeBones(24, [40, 32], [32, 40])
    with pytest.raises(NotImplementedError, match="Pose3DVaeBones"):
        models.Pose3DVaeCat(24, [40, 32], [32, 40], pose3d=lifter, pred_bones=True)
    with pytest.raises(NotImplementedError, match="Pose3DVaeBones"):
        models.Pose3DVae(24, [40, 32], [32, 40], pose3d=lifter, pred_bones=True)
    with pytest.raises(ValueError):
        pv.vae.filter_sequences(out_3d, [0, 150])
    pv.close()
    # use_2d alone: the 96-input filter over [x2d, bones]; bones alone: the 64-input filter
    for use_2d, n_in in ((True, 96), (False, 64)):
        p2 = models.Pose3DVaeBones(24, [40, 32], [32, 40], use_2d=use_2d, pose3d=lifter, max_batch=256, seed=3)
        s2 = (n_in, (40, 32), 24, (32, 40))
        assert p2.vae.input_size == n_in
        P2 = rand_params(s2, 22)
        p2.vae.set_weights(P2)
        o3d, (m2, c2) = p2(xd, eps=eps)
        bb = vb.bones_from_joints(o3d.cpu().numpy(), np.float64)
        c = vb.forward(P2, s2, np.concatenate([x, bb], axis=1) if use_2d else bb, eps)
        close(m2.cpu().numpy(), c["mag"], "mag %d" % n_in)
        close(c2.cpu().numpy(), c["cos"], "cos %d" % n_in)
        with pytest.raises(ValueError):
            p2(xd, effnet_output=F[:150], eps=eps)
        p2.close()
    lifter.close()


def test_driver_trains_two_epochs(tmp_path):
    """pose_3d_bones.train() on synthetic H3.6M archives and a synthetic feature archive: the frozen
    lifter restored from a predict_3dpose.train checkpoint, two epochs at train.yml's factors;
    histories finite, the mean training loss falls from epoch 1 to epoch 2, the lifter unchanged, the
    weights saved under the bones names."""
    import predict_3dpose
    sys.path.insert(0, os.path.join(HERE, "golden"))
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
        "pose_3d_bones", os.path.join(os.path.dirname(HERE), "3d-pose-baseline_amd", "pose_3d_bones.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    cfg = tmp_path / "train.yml"
    cfg.write_text("train:\n  step_log: 2000\n  learning_rate: 0.0001\n  mag_factor: 10.0\n  cos_factor: 100.0\n"
                   "  ang_factor: 100.0\n  dkl_factor: 1.0\n")
    common = data + net + ["--cfg_file", str(cfg), "--train_dir", str(tmp_path / "vae"), "--effnet_outputs_path", feats,
                           "--load", str(step), "--lifter_dir", predict_3dpose.train_dir_for(lflags),
                           "--bones_mapping_dir", os.path.join(HERE, "golden", "bones_mapping.yml")]
    model, hist = drv.train(common + ["--epochs", "2", "--use_effb1"], read_from_config=True)
    assert drv.ENV.FLAGS.learning_rate == 1e-4 and drv.ENV.FLAGS.cos_factor == 100.0
    for k, v in model.pose3d.get_weights().items():
        np.testing.assert_array_equal(v, lw[k], err_msg=k)
    for key in ("loss_train", "loss_test", "error_3d_out", "error_vae_out"):
        assert len(hist[key]) == 2 and np.isfinite(np.asarray(hist[key], np.float64)).all(), key
    assert np.asarray(hist["loss_train"]).shape == (2, 4)
    print("train loss per epoch", hist["loss_train"], "test loss per epoch", hist["loss_test"],
          "errors", hist["error_3d_out"], hist["error_vae_out"])
    assert hist["loss_train"][1].sum() < hist["loss_train"][0].sum()
    assert model.vae.get_step()[0] > 0 and model.vae.input_size == 1376
    saved = os.path.join(drv.ENV.TRAIN_DIR, "3d_effnet_2d_vae_bones", "last_model_weights.npz")
    assert os.path.isfile(os.path.join(drv.ENV.TRAIN_DIR, "3d_effnet_2d_vae_bones", "train.cfg"))
    with np.load(saved) as z:
        assert sorted(z.files) == sorted(n for n, _ in vb.param_names(SHAPES["wide1376"]))
        assert z["enc_h_40/kernel"].shape == (1376, 40)
        for (n, _, _), w in zip(model.vae.param_table, model.vae.get_weights()):
            np.testing.assert_array_equal(z[n], w)
    for flag, exc in ((["--train_all"], NotImplementedError), (["--sample"], NotImplementedError),
                      (["--optimizer", "rmsprop"], NotImplementedError)):
        with pytest.raises(exc):
            drv.train(common + ["--epochs", "1"] + flag)
    model.close()
    model.pose3d.close()
