"""What the references do with non-finite input rows (no GPU): the conditions that
tests/test_gpu_nonfinite.py holds the HIP kernels to.

For every oracle: the bad rows come out NaN in every column, every other row has the bits of the
twin's run (tests/nonfinite_cases.py), losses are NaN and every gradient element is NaN.  Where an
input did not satisfy these on the reference alone, the input would be changed, not the assertion.
"""
import numpy as np
import pytest

import clip_oracle
import nonfinite_cases as nc
import vae_oracle as vo
import vae_seq_oracle as so
from oracle import ref_eval, ref_frontend, ref_mlp


@pytest.mark.parametrize("name", list(nc.LIFTER_CASES))
def test_lifter_forward_rows(name):
    """Every case the GPU forms run (ref_mlp.forward; bf16_*: the emulated-bf16 oracle)."""
    k = nc.lifter_case(name)
    cfg, st, B, bad, twin, mask, yb, yt = (k[n] for n in ("cfg", "st", "B", "bad", "twin", "mask", "ref_bad", "ref_twin"))
    assert yb.shape == (B, cfg.output_size) and mask[2 if B == 4 else B - 1] and (B == 1 or not mask.all())
    nc.check_rows(yb, yt, mask, "oracle forward")
    if B >= 37:   # every kind of poison is there
        kinds = {("nan" if np.isnan(r).all() else "nan1" if np.isnan(r).any() else "inf" if np.isposinf(r).any() else "ninf")
                 for r in bad[mask]}
        assert kinds == {"nan", "nan1", "inf", "ninf"}
    if name.startswith("bf16"):
        return
    t = np.random.default_rng(B + 1).standard_normal((B, cfg.output_size)).astype(np.float32)
    loss, _ = ref_mlp.eval_step(st, bad, t)
    assert np.isnan(loss)
    assert np.isfinite(ref_mlp.eval_step(st, twin, t)[0])
    # a NaN in the target alone: the outputs are the twin's, the loss is NaN
    tb = t.copy()
    tb[B // 2, 3] = np.nan
    loss_t, y_t = ref_mlp.eval_step(st, twin, tb)
    assert np.isnan(loss_t)
    np.testing.assert_array_equal(y_t, yt)


@pytest.mark.parametrize("bn", [True, False])
@pytest.mark.parametrize("B", [64, 17])
def test_lifter_training_step(bn, B):
    """One NaN element in x at keep 0.5: NaN loss, every gradient element NaN, all output rows NaN
    under batch norm (the batch statistics carry it) and only the bad row without; after the step
    the moving statistics, every weight and both Adam slots are NaN throughout."""
    cfg = ref_mlp.Cfg(linear_size=256, num_layers=2, residual=True, batch_norm=bn)
    st = ref_mlp.init_state(cfg, seed=4, bn_seed=5)
    rng = np.random.default_rng(B)
    x = rng.standard_normal((B, 32)).astype(np.float32)
    t = rng.standard_normal((B, 48)).astype(np.float32)
    x[B - 1, 7] = np.nan
    out, cache = ref_mlp.forward(st, x, True, 0.5, seed=9, ctr=0)
    loss, dy = ref_mlp.mse(out, t)
    grads = ref_mlp.backward(st, cache, dy)
    assert np.isnan(loss)
    want = np.ones(B, bool) if bn else np.arange(B) == B - 1
    np.testing.assert_array_equal(np.isnan(out).all(axis=1), want)
    np.testing.assert_array_equal(np.isnan(out).any(axis=1), want)
    assert sorted(grads) == sorted(n for n, _ in ref_mlp.param_names(cfg))
    for name, g in grads.items():
        assert nc.all_nan(g), name
    loss2, _ = ref_mlp.train_step(st, x, t, 0.5, 1e-3, seed=9, ctr=0)
    assert np.isnan(loss2)
    for k, v in st.moving.items():
        assert nc.all_nan(v), k
    for name, _ in ref_mlp.param_names(cfg):
        assert nc.all_nan(st.params[name]) and nc.all_nan(st.m[name]) and nc.all_nan(st.v[name]), name
    # a NaN in the target alone poisons the loss and every gradient too: the output layer's in that
    # output column, everything below it throughout
    x[B - 1, 7] = 0.25
    t[0, 0] = np.nan
    st = ref_mlp.init_state(cfg, seed=4, bn_seed=5)
    out, cache = ref_mlp.forward(st, x, True, 0.5, seed=9, ctr=0)
    loss, dy = ref_mlp.mse(out, t)
    assert np.isnan(loss) and not np.isnan(out).any()
    for name, g in ref_mlp.backward(st, cache, dy).items():
        if name in ("linear_model/w4", "linear_model/b4"):
            col = np.isnan(g).reshape(-1, 48)
            assert col[:, 0].all() and not col[:, 1:].any(), name
        else:
            assert nc.all_nan(g), name


@pytest.mark.parametrize("name", ["default", "edge264", "wide"])
def test_vae_rows_losses_and_gradients(name):
    k = nc.vae_case(name, 17, [16], seed=17)
    shape = k["shape"]
    P = nc.vae_params(shape, 3)
    cb = vo.forward(P, shape, k["x_bad"], k["eps"])
    ct = vo.forward(P, shape, k["x"], k["eps"])
    for key in ("y", "mean", "log_var", "z"):
        nc.check_rows(cb[key], ct[key], k["mask"], key)
    terms = vo.row_terms(cb, k["t"])
    nc.check_rows(terms, vo.row_terms(ct, k["t"]), k["mask"], "row_terms")
    assert nc.all_nan(vo.loss3(terms, nc.VAE_FACTORS))
    g, _ = vo.backward(P, shape, cb, k["t"], nc.VAE_FACTORS)
    assert sorted(g) == sorted(P)
    for n, v in g.items():
        assert nc.all_nan(v), n
    # a NaN in the target alone: the forward is the twin's, the loss and gradients that see t are NaN
    tb = k["t"].copy()
    tb[3, 4] = np.nan
    terms = vo.row_terms(ct, tb)
    loss = vo.loss3(terms, nc.VAE_FACTORS)
    assert np.isnan(loss[0]) and np.isnan(loss[1]) and np.isfinite(loss[2])
    g, _ = vo.backward(P, shape, ct, tb, nc.VAE_FACTORS)
    for n, v in g.items():
        assert nc.all_nan(v), n


def test_vae_sequence_filter_poisons_the_rest_of_its_sequence():
    shape = nc.VAE_SHAPES["edge96"]
    P = nc.vae_params(shape, 3)
    k = nc.seq_case(shape, nc.SEQ_LENS, nc.SEQ_BAD, seed=96)
    rb = so.filter(P, shape, k["pred_bad"], k["off"], k["eps"], target=k["tgt"])
    rt = so.filter(P, shape, k["pred"], k["off"], k["eps"], target=k["tgt"])
    nc.check_rows(rb["ref"], rt["ref"], k["mask"], "ref")
    nc.check_rows(rb["frame_err"][:, 1], rt["frame_err"][:, 1], k["mask"], "err_ref")
    nc.check_rows(rb["seq_err"][:, 1], rt["seq_err"][:, 1], k["seq_mask"], "seq_err")
    # frames before the poisoned one are untouched: the mask starts at frame k, not at the sequence's first
    s, f = 5, nc.SEQ_BAD[5]
    assert f > 0 and not k["mask"][k["off"][s]:k["off"][s] + f].any() and k["mask"][k["off"][s] + f]
    assert 0 < k["mask"].sum() < k["N"]


@pytest.mark.parametrize("smooth", [True, False])
def test_clip_composition_spreads_a_nan_keypoint_over_its_window(smooth):
    """clip_oracle.smooth -> the front end's per-frame lift -> clip_oracle.post: one NaN keypoint
    makes every frame of its median window a NaN pose (every predicted coordinate), no other."""
    n, frame, col = 23, 11, 5
    bad, twin = nc.clip_case(n, 23, frame, col)
    cfg = ref_mlp.Cfg(linear_size=256, num_layers=1, residual=True, batch_norm=True)
    st = ref_mlp.init_state(cfg, seed=3, bn_seed=4)
    s = ref_eval.synthetic_stats()
    rng = np.random.default_rng(5)
    mean2, std2 = rng.uniform(200, 600, 64), rng.uniform(50, 150, 64)
    mean3, std3 = rng.uniform(-400, 400, 96), rng.uniform(30, 300, 96)
    mask = nc.window_frames(n, frame, smooth)
    assert mask.sum() == (7 if smooth else 1)
    res = []
    for xy in (bad, twin):
        xy_s = clip_oracle.smooth(xy, smooth=smooth)
        un, norm = ref_frontend.lift_frames(st, xy_s, mean2, std2, s["use2"], mean3, std3, s["ign3"])
        poses, src = clip_oracle.post(un, xy_s, cache_on_fail=False)
        res.append((xy_s, norm, poses))
    np.testing.assert_array_equal(np.isnan(res[0][0]).any(axis=1), mask)
    nc.check_rows(res[0][1], res[1][1], mask, "network rows")
    used = np.zeros(96, bool)
    used.reshape(32, 3)[np.asarray(s["use3"]).reshape(-1, 3)[:, 0] // 3] = True     # the predicted joints' coordinates
    nc.check_rows(res[0][2][:, used], res[1][2][:, used], mask, "poses")


def test_bf16_rounding_keeps_nan_and_inf():
    bits = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFF80FFFF, 0x7F808000, 0x7F800000, 0xFF800000,
                     0x3F808000, 0x3F818000, 0x7F7FFFFF], np.uint32)
    r = ref_mlp.bf16_round(bits.view(np.float32))
    assert r.dtype == np.float32 and r.shape == bits.shape
    assert np.isnan(r[:6]).all(), r[:6]
    assert r[6] == np.inf and r[7] == -np.inf
    # ties to even, and a finite value past the largest bf16 rounds to Inf as IEEE rounding does
    np.testing.assert_array_equal(r[8:].view(np.uint32), np.array([0x3F800000, 0x3F820000, 0x7F800000], np.uint32))


def test_mpjpe_sum_with_a_nan_prediction_row():
    """ref_eval.batch_dists: a NaN prediction row makes the per-joint sums of the predicted joints
    NaN; the root joint (not predicted: its coordinates are the statistics' on both sides) stays 0."""
    s = ref_eval.synthetic_stats()
    pred, twin, mask = nc.poisoned((70, 48), [33], seed=70, kinds=("nan_row",))
    gt = np.random.default_rng(71).standard_normal((70, 48))
    d = ref_eval.batch_dists(pred, gt, s["mean3"], s["std3"], s["ign3"], s["use3"]).sum(axis=0)
    assert d.shape == (17,) and d[0] == 0.0 and np.isnan(d[1:]).all()
    dt = ref_eval.batch_dists(twin, gt, s["mean3"], s["std3"], s["ign3"], s["use3"]).sum(axis=0)
    assert np.isfinite(dt).all()
