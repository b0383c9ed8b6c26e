"""Non-finite input rows through every device path, against the oracles ("Non-finite
input"): a row holding a NaN or an Inf leaves every forward as a NaN row and makes the loss and
every gradient NaN, as np.maximum and the mask products of the oracles do; no other row changes by
a bit; and NaN data is not a failed launch (the error flags stay clean).

Each forward form runs the poisoned input first and then its finite twin ON THE SAME MODEL OBJECT,
so a hand-off slot, workspace row or epilogue table left poisoned would show in the twin's rows.
Per form (tests/nonfinite_cases.py; the same inputs pass tests/test_nonfinite_oracle.py on the
references alone):

1. the bad rows are NaN in every output column, and so are the oracle's;
2. every good row equals the twin's row from the same form bit for bit (a padded tail row that
   repeats a NaN last row, a 0 * NaN of a masked lane or a poisoned shared tile would show);
3. the twin's rows are within the sibling tests' bound of the fp64 oracle: 2e-5 + 2e-5 |ref|, or
   5e-5 where the sibling test of that form uses it;
4. p3d_error_flags is 0 and serve_check() is clean.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import _p3d  # noqa: E402
import clip_oracle  # noqa: E402
import data_utils  # noqa: E402
import linear_model  # noqa: E402
import nonfinite_cases as nc  # noqa: E402
import openpose_frontend as of  # noqa: E402
import predict_3dpose  # noqa: E402
import vae_oracle as vo  # noqa: E402
import vae_seq_oracle as so  # noqa: E402
from oracle import ref_eval, ref_frontend, ref_mlp  # noqa: E402
from top_vae_3d_pose import models  # noqa: E402


def make(k, max_batch=None, batch=64, dtype=None, lr=1e-3, model_seed=11):
    cfg = k["cfg"]
    m = linear_model.LinearModel(cfg.linear_size, cfg.num_layers, cfg.residual, cfg.batch_norm, cfg.max_norm,
                                 batch, lr, "/tmp/p3d_test", cfg.predict_14, dtype, seed=model_seed,
                                 max_batch=max_batch or max(batch, 64))
    m.set_weights({**k["st"].params, **k["st"].moving})
    return m


def close(a, b, tol=2e-5, what=""):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b)
    bound = tol + tol * np.abs(b)
    print("%s max |err| %.3g" % (what, err.max()))
    assert np.all(err <= bound), "%s max err %.3g (at ref %.3g)" % (what, err.max(), b.flat[np.argmax(err - bound)])


def kname(m):
    name = ctypes.create_string_buffer(128)
    _p3d.check(_p3d.lib().p3d_kernel_name(m._h, 3, name, 128), "p3d_kernel_name")
    return name.value.decode()


def tags_of(m, fn):
    _p3d.check(_p3d.lib().p3d_profile_start(m._h, 64), "p3d_profile_start")
    out = fn()
    buf = ctypes.create_string_buffer(1 << 12)
    _p3d.check(_p3d.lib().p3d_profile_stop(m._h, buf, len(buf)), "p3d_profile_stop")
    return out, {ln.split("\t")[0]: int(ln.split("\t")[1]) for ln in buf.value.decode().strip().splitlines()}


def clean(m):
    """Assertion 4: NaN data set no error flag."""
    torch.cuda.synchronize()
    f = ctypes.c_int32(-1)
    _p3d.check(_p3d.lib().p3d_error_flags(m._h, ctypes.byref(f), 0), "p3d_error_flags")
    assert f.value == 0, f.value
    m.check_errors()
    m.serve_check()


def check_form(m, run, k, tol, what):
    """Assertions 1-4 for one forward form: run(x numpy [B, 32]) -> y numpy, poisoned input first."""
    yb = run(k["bad"])
    yt = run(k["twin"])
    nc.check_rows(k["ref_bad"], k["ref_twin"], k["mask"], what + " (oracle)")
    nc.check_rows(yb, yt, k["mask"], what)
    close(yt, k["ref_twin"], tol, what)
    clean(m)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------
# the lifter's forward forms
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["L64_B1", "L64_B4", "L1024_B1", "L1024_B4"])
@pytest.mark.parametrize("form", ["chain", "fold", "plain", "mfma"])
def test_small_batch_forms(case, form, monkeypatch):
    """Batch <= 4: k_gemv_chain, the four-launch fold (P3D_GEMV_CHAIN=0), the plain launches
    (P3D_GEMV_FOLD=0) and the 16-row MFMA kernels (P3D_GEMV_MAXB=0)."""
    env = {"chain": {}, "fold": {"P3D_GEMV_CHAIN": "0"}, "plain": {"P3D_GEMV_FOLD": "0"}, "mfma": {"P3D_GEMV_MAXB": "0"}}[form]
    for key in ("P3D_GEMV_CHAIN", "P3D_GEMV_FOLD", "P3D_GEMV_MAXB"):
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    k = nc.lifter_case(case)
    m = make(k, batch=k["B"], max_batch=64)
    L, N = k["cfg"].linear_size, k["cfg"].num_layers
    seen = []

    def run(x):
        y, tags = tags_of(m, lambda: m.forward_device(dev(x), False, 1.0).cpu().numpy())
        seen.append(tags)
        return y

    check_form(m, run, k, 2e-5, "%s %s" % (form, case))
    fold = {"gemv_in_hidden": 1, "gemv_hidden_out": 1, "gemv_hidden": 2 * N - 2}
    fits = 2 * N * (L // 16) <= torch.cuda.get_device_properties(0).multi_processor_count
    want = {"chain": {"gemv_chain": 1} if fits else fold, "fold": fold,
            "plain": {"gemv_in": 1, "gemv_hidden": 2 * N, "gemv_out": 1}}.get(form)
    for tags in seen:
        if want is not None:
            assert tags == want, (form, tags)
        else:
            assert tags and not any(t.startswith("gemv") for t in tags), tags
    m.close()


@pytest.mark.parametrize("case", ["bn_B37", "bn_B200", "nobn_B37", "nobn_B200", "maxnorm_B37", "maxnorm_B200",
                                  "p14_B37", "p14_B200"])
def test_batch64_layer_kernels(case):
    """forward_device below the large-M threshold: the 16x16-tile layer kernels (tags fwd_in /
    fwd_hidden / fwd_out), ragged row tiles, every epilogue variant."""
    k = nc.lifter_case(case)
    m = make(k, batch=k["B"], max_batch=max(k["B"], 64))
    seen = []

    def run(x):
        y, tags = tags_of(m, lambda: m.forward_device(dev(x), False, 1.0).cpu().numpy())
        seen.append(tags)
        return y

    check_form(m, run, k, 5e-5, case)
    for tags in seen:
        assert tags and all(t.startswith("fwd_") and "big" not in t and "train" not in t for t in tags), tags
    m.close()


def test_large_m_gemm():
    """k_gemm_f32 (M >= 256; tags fwd_in_big / fwd_hidden_big): 128-row tiles, a ragged last one."""
    k = nc.lifter_case("gemm_B300")
    m = make(k, batch=64, max_batch=300)
    seen = []

    def run(x):
        y, tags = tags_of(m, lambda: m.forward_device(dev(x), False, 1.0).cpu().numpy())
        seen.append(tags)
        return y

    check_form(m, run, k, 5e-5, "gemm_B300")
    for tags in seen:
        assert "fwd_hidden_big" in tags, tags
    m.close()


SERVE_FORMS = [
    # (id, case, env, kernel-name test, bound)
    ("serve5_L256", "serve_L256_B327", {"P3D_SERVE6": "0"}, lambda n: n.startswith("k_serve5"), 2e-5),
    ("serve5_L384", "serve_L384_B327", {"P3D_SERVE6": "0"}, lambda n: n.startswith("k_serve5"), 2e-5),
    ("serve6_B327", "serve_L1024_B327", {}, lambda n: n.startswith("k_serve6<"), 2e-5),
    ("serve6_B1280", "serve_L1024_B1280", {}, lambda n: n.startswith("k_serve6<"), 2e-5),
    ("serve6_split3_B327", "serve_L1024_B327", {"P3D_SERVE6_SPLIT": "3", "P3D_SERVE6_RT": "4"},
     lambda n: n.startswith("k_serve6<"), 5e-5),
    ("serve6_split3_B1280", "serve_L1024_B1280", {"P3D_SERVE6_SPLIT": "3", "P3D_SERVE6_RT": "4"},
     lambda n: n == "k_serve6<2, 3, 7, 4>", 5e-5),
    ("rounds_B2112", "rounds_B2112", {}, lambda n: n == "k_serve6_rounds<4, 3, 2, 5>", 5e-5),
]


@pytest.mark.parametrize("fid,case,env,name_ok,tol", SERVE_FORMS, ids=[f[0] for f in SERVE_FORMS])
def test_serve_forms(fid, case, env, name_ok, tol, monkeypatch):
    """p3d_serve on k_serve5, k_serve6 (the default choice and one forced split) and
    k_serve6_rounds (bad rows in the first round, in the last round and in its 32-row tail)."""
    for key in ("P3D_SERVE6", "P3D_SERVE6_SPLIT", "P3D_SERVE6_RT", "P3D_SERVE6_PAIR", "P3D_SERVE6_MAX_NB"):
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    k = nc.lifter_case(case)
    m = make(k)
    for key in env:
        monkeypatch.delenv(key)
    names = []

    def run(x):
        y = m.serve_device(dev(x)).cpu().numpy()
        names.append(kname(m))
        return y

    check_form(m, run, k, tol, fid)
    assert all(name_ok(n) for n in names), names
    m.close()


@pytest.mark.parametrize("case", ["L1024_B37", "L1024_B4"])
@pytest.mark.parametrize("sync", [False, True])
def test_serve_mse(case, sync):
    """p3d_serve_mse / p3d_serve_mse_sync: NaN rows and a NaN loss; the twin's loss within 1e-5
    relative of the oracle's; a NaN in t alone leaves y the twin's bits and makes the loss NaN."""
    k = nc.lifter_case(case)
    B, st = k["B"], k["st"]
    m = make(k)
    c, lib = ctypes.c_void_p, _p3d.lib()
    fn = lib.p3d_serve_mse_sync if sync else lib.p3d_serve_mse
    t = np.random.default_rng(B + 5).standard_normal((B, 48)).astype(np.float32)
    t_bad = t.copy()
    t_bad[B // 2, 47] = np.nan
    hx = torch.empty((B, 32), dtype=torch.float32).pin_memory()
    ht = torch.empty((B, 48), dtype=torch.float32).pin_memory()
    hy = torch.empty((B, 48), dtype=torch.float32).pin_memory()
    hl = torch.zeros(4, dtype=torch.float32).pin_memory()

    def run(x, tt):
        hx.copy_(torch.from_numpy(np.ascontiguousarray(x)))
        ht.copy_(torch.from_numpy(tt))
        hy.zero_()
        hl.zero_()
        _p3d.check(fn(m._h, c(hx.data_ptr()), B, c(hy.data_ptr()), c(ht.data_ptr()), c(hl.data_ptr()),
                      c(_p3d.stream_handle())), "p3d_serve_mse")
        torch.cuda.synchronize()
        return hy.numpy().copy(), float(hl[0])

    yb, lb = run(k["bad"], t)
    yt, lt = run(k["twin"], t)
    yn, ln = run(k["twin"], t_bad)
    assert np.isnan(ref_mlp.eval_step(st, k["bad"], t)[0]) and np.isnan(ref_mlp.eval_step(st, k["twin"], t_bad)[0])
    nc.check_rows(k["ref_bad"], k["ref_twin"], k["mask"], "oracle")
    nc.check_rows(yb, yt, k["mask"], case)
    assert np.isnan(lb), lb
    close(yt, k["ref_twin"], 2e-5, case)
    rl = ref_mlp.eval_step(st, k["twin"], t)[0]
    assert abs(lt - rl) <= 1e-5 * max(1.0, abs(rl)), (lt, rl)
    np.testing.assert_array_equal(yn, yt)
    assert np.isnan(ln), ln
    clean(m)
    # the reference's eval step() from numpy (the same launch behind LinearModel.step): NaN loss, not an error
    loss, _, out = m.step(None, np.array(k["bad"], np.float64), t.astype(np.float64), 1.0, isTraining=False)
    assert np.isnan(loss)
    nc.check_rows(out, yt, k["mask"], "step")
    clean(m)
    m.close()


def test_bf16_forward():
    """The bf16 path vs the emulated-bf16 oracle (whose rounding keeps NaN): the bounds of
    test_bf16_inference_matches_emulated_oracle at L <= 512 (max 1e-3, mean 1e-5 of the range)."""
    k = nc.lifter_case("bf16_B200")
    B = k["B"]
    m = make(k, batch=B, max_batch=B, dtype="bfloat16", model_seed=3)
    yb = m.forward_device(dev(k["bad"])).cpu().numpy()
    yt = m.forward_device(dev(k["twin"])).cpu().numpy()
    nc.check_rows(k["ref_bad"], k["ref_twin"], k["mask"], "bf16 (oracle)")
    nc.check_rows(yb, yt, k["mask"], "bf16")
    scale = np.abs(k["ref_twin"]).max()
    err = np.abs(yt - k["ref_twin"])
    assert err.max() <= 1e-3 * scale and err.mean() <= 1e-5 * scale, (err.max(), err.mean(), scale)
    clean(m)
    m.close()


# ------------------------------------------------------------------------------------------------
# the front end: FrameLifter / p3d_lift, ClipLifter, the MPJPE accumulator
# ------------------------------------------------------------------------------------------------

USE2, _ = data_utils.dimension_sets(2)
USE3, IGN3 = data_utils.dimension_sets(3)


def front_setup(seed=3):
    rng = np.random.default_rng(seed)
    cfg = ref_mlp.Cfg(linear_size=1024, num_layers=2, residual=True, batch_norm=True)
    st = ref_mlp.init_state(cfg, seed=seed, bn_seed=seed + 1)
    m = linear_model.LinearModel(1024, 2, True, True, False, 64, 1e-3, "/tmp/p3d_fe", seed=11)
    m.set_weights({**st.params, **st.moving})
    s = dict(mean2=rng.uniform(200, 600, 64), std2=rng.uniform(50, 150, 64),
             mean3=rng.uniform(-400, 400, 96), std3=rng.uniform(30, 300, 96))
    return st, m, s


@pytest.mark.parametrize("B", [1, 4])
def test_frame_lifter(B):
    """FrameLifter / p3d_lift at batch 1 (the whole pose NaN) and 4 (frame 2 bad): every predicted
    coordinate of a bad frame is NaN, the coordinates the network does not predict are the
    statistics' means as ever, the other frames have the twin's bits."""
    st, m, s = front_setup()
    rng = np.random.default_rng(40 + B)
    twin = rng.uniform(100, 900, (B, 36))
    bad = twin.copy()
    row = 0 if B == 1 else 2
    bad[row, 7] = np.nan                      # one keypoint coordinate
    mask = np.arange(B) == row
    fl = of.FrameLifter(m, s["mean2"], s["std2"], USE2, s["mean3"], s["std3"], IGN3, batch=B)
    gb = fl.lift(bad)
    gt = fl.lift(twin)
    args = (s["mean2"], s["std2"], USE2, s["mean3"], s["std3"], IGN3)
    _, norm_bad = ref_frontend.lift_frames(st, bad, *args)
    _, norm_twin = ref_frontend.lift_frames(st, twin, *args)
    nc.check_rows(norm_bad, norm_twin, mask, "front end (oracle)")
    nc.check_rows(gb[:, USE3], gt[:, USE3], mask, "FrameLifter")
    np.testing.assert_array_equal(gb[:, IGN3], np.tile(s["mean3"][IGN3], (B, 1)))
    norm = (gt[:, USE3] - s["mean3"][USE3]) / s["std3"][USE3]
    close(norm, norm_twin, 2e-5, "FrameLifter")
    clean(m)
    m.close()


@pytest.mark.parametrize("smooth", [True, False])
def test_clip_lifter(smooth):
    """ClipLifter.lift_clip, 23 frames, one NaN keypoint: p3d_clip_prepare keeps it and (smoothing
    on) spreads it over its median window, the lifter makes those frames NaN rows, p3d_clip_finish
    keeps them -- as clip_oracle.smooth -> the oracle's front end -> clip_oracle.post do."""
    n, frame, col = 23, 11, 5
    bad, twin = nc.clip_case(n, 23, frame, col)
    mask = nc.window_frames(n, frame, smooth)
    st, m, s = front_setup()
    cl = of.ClipLifter(m, s["mean2"], s["std2"], USE2, s["mean3"], s["std3"], IGN3, max_frames=n + 3, cache_on_fail=False)
    res, rows = [], []
    for xy in (bad, twin):
        res.append(cl.lift_clip(xy, smooth=smooth))
        rows.append(cl.network_rows(n).cpu().numpy().astype(np.float64))
    want = []
    for xy in (bad, twin):
        xy_s = clip_oracle.smooth(xy, smooth=smooth)
        un, norm = ref_frontend.lift_frames(st, xy_s, s["mean2"], s["std2"], USE2, s["mean3"], s["std3"], IGN3)
        want.append((xy_s, norm, clip_oracle.post(un, xy_s, cache_on_fail=False)))
    for (poses, xy_s, src), (w_s, _, (w_poses, w_src)) in zip(res, want):
        np.testing.assert_array_equal(xy_s, w_s)                      # (NaN == NaN here)
        np.testing.assert_array_equal(src, w_src)
        np.testing.assert_array_equal(np.isnan(poses), np.isnan(w_poses))
    np.testing.assert_array_equal(np.isnan(res[0][1]).any(axis=1), mask)
    nc.check_rows(want[0][1], want[1][1], mask, "network rows (oracle)")
    nc.check_rows(rows[0], rows[1], mask, "network rows")
    close(rows[1], want[1][1], 2e-5, "network rows")
    pose_nan = np.isnan(want[0][2][0])
    np.testing.assert_array_equal(pose_nan.any(axis=1), mask)
    np.testing.assert_array_equal(res[0][0][~mask], res[1][0][~mask])
    assert pose_nan[mask].sum() >= 48 * mask.sum()                   # every predicted coordinate
    clean(m)
    m.close()


def test_mpjpe_accumulator():
    """p3d_mpjpe_accum, plain protocol: one NaN prediction row makes the accumulated per-joint sums
    NaN where ref_eval's are (every predicted joint; the root joint stays 0)."""
    stats = ref_eval.synthetic_stats()
    pred, twin, mask = nc.poisoned((70, 48), [33], seed=70, kinds=("nan_row",))
    gt = np.random.default_rng(71).standard_normal((70, 48)).astype(np.float32)
    m = linear_model.LinearModel(256, 1, True, True, False, 64, 1e-3, "/tmp/p3d_test", seed=1)
    sums = []
    for p in (pred, twin):
        acc = predict_3dpose.MPJPE(m, stats["mean3"], stats["std3"], stats["use3"])
        acc.add(dev(p), dev(gt))
        sums.append(acc.joint_sum.cpu().numpy())
    ref = [ref_eval.batch_dists(p, gt.astype(np.float64), stats["mean3"], stats["std3"], stats["ign3"],
                                stats["use3"]).sum(axis=0) for p in (pred, twin)]
    assert np.isnan(ref[0][1:]).all() and ref[0][0] == 0.0
    np.testing.assert_array_equal(np.isnan(sums[0]), np.isnan(ref[0]))
    assert sums[0][0] == 0.0
    np.testing.assert_allclose(sums[1], ref[1], rtol=1e-12, atol=1e-9)
    clean(m)
    m.close()


# ------------------------------------------------------------------------------------------------
# the VAE filter
# ------------------------------------------------------------------------------------------------

def vae_close(got, ref, what):
    close(got, ref, 2e-5, what)


_vae = {}


def vae_model(name, max_batch=64):
    if name not in _vae:
        shape = nc.VAE_SHAPES[name]
        m = models.VAE(shape[0], shape[2], shape[1], shape[3], shape[4], max_batch=max_batch, seed=5)
        m.set_weights(nc.vae_params(shape, 3))
        _vae[name] = m
    return _vae[name]


def vae_forward_check(m, k, xin_bad, xin_twin, what):
    shape = k["shape"]
    P = nc.vae_params(shape, 3)
    keys = ("y", "mean", "log_var", "z")
    ob = m.forward_device(xin_bad, eps=k["eps"], target=k["t"], want=keys)
    lb = m.loss_device(xin_bad, k["t"], nc.VAE_FACTORS, eps=k["eps"]).cpu().numpy().copy()
    ot = m.forward_device(xin_twin, eps=k["eps"], target=k["t"], want=keys)
    lt = m.loss_device(xin_twin, k["t"], nc.VAE_FACTORS, eps=k["eps"]).cpu().numpy().copy()
    cb = vo.forward(P, shape, k["x_bad"], k["eps"])
    ct = vo.forward(P, shape, k["x"], k["eps"])
    for key in keys:
        nc.check_rows(cb[key], ct[key], k["mask"], what + " oracle " + key)
        nc.check_rows(ob[key].cpu().numpy(), ot[key].cpu().numpy(), k["mask"], what + " " + key)
        vae_close(ot[key].cpu().numpy(), ct[key], what + " " + key)
    tb, tt = vo.row_terms(cb, k["t"]), vo.row_terms(ct, k["t"])
    nc.check_rows(tb, tt, k["mask"], what + " oracle row_terms")
    nc.check_rows(ob["row_terms"].cpu().numpy(), ot["row_terms"].cpu().numpy(), k["mask"], what + " row_terms")
    vae_close(ot["row_terms"].cpu().numpy(), tt, what + " row_terms")
    assert nc.all_nan(vo.loss3(tb, nc.VAE_FACTORS)) and nc.all_nan(lb), lb
    np.testing.assert_allclose(lt, vo.loss3(tt, nc.VAE_FACTORS), rtol=1e-5, atol=0)
    torch.cuda.synchronize()


def test_vae_narrow_forward_and_loss():
    k = nc.vae_case("default", 17, [16], seed=17)
    vae_forward_check(vae_model("default"), k, k["x_bad"], k["x"], "narrow")


@pytest.mark.parametrize("name", ["edge264", "wide"])
def test_vae_wide_forward_and_loss(name):
    k = nc.vae_case(name, 17, [16], seed=17, kinds=("nan_last",))
    vae_forward_check(vae_model(name), k, k["x_bad"], k["x"], name)


@pytest.mark.parametrize("name", ["edge264", "wide"])
def test_vae_wide_table_input(name):
    """The (table, idx) form: the NaN sits in a table row that two batch rows index (3 and 16, the
    last row); the rows that index other table rows keep the twin's bits."""
    shape = nc.VAE_SHAPES[name]
    B, rows_t = 17, 9
    w2 = shape[0] - 80
    rng = np.random.default_rng(5 + shape[0])
    a, b = (rng.standard_normal((B, w)).astype(np.float32) for w in (32, 48))
    table = rng.standard_normal((rows_t, w2)).astype(np.float32)
    idx = rng.integers(0, rows_t - 1, size=B)      # row rows_t - 1 is indexed by rows 3 and 16 alone
    idx[3] = idx[16] = rows_t - 1
    table_bad = table.copy()
    table_bad[rows_t - 1, w2 - 1] = np.nan
    mask = np.zeros(B, bool)
    mask[[3, 16]] = True
    k = dict(shape=shape, mask=mask, x=np.concatenate([a, b, table[idx]], axis=1),
             x_bad=np.concatenate([a, b, table_bad[idx]], axis=1),
             t=rng.standard_normal((B, 48)).astype(np.float32), eps=rng.standard_normal((B, shape[2])).astype(np.float32))
    idx_d = dev(idx.astype(np.int64))
    segs = lambda tb: [dev(a), dev(b), (dev(tb), idx_d)]     # noqa: E731
    vae_forward_check(vae_model(name), k, segs(table_bad), segs(table), name + " table")


@pytest.mark.parametrize("form", [0, 1])
def test_vae_sequence_filter(form):
    """p3d_vae_seq_filter on the smallest shape of tests/test_gpu_vae_seq.py: each refined frame is
    fed back, so one NaN frame poisons the rest of its sequence and nothing else -- sequences at
    tile positions 5 (first 16-sequence tile), 0 and 3 (second tile)."""
    shape = nc.VAE_SHAPES["edge96"]
    P = nc.vae_params(shape, 3)
    m = vae_model("edge96")
    k = nc.seq_case(shape, nc.SEQ_LENS, nc.SEQ_BAD, seed=96)
    want = ("ref", "frame_err", "seq_err")
    m.set_seq_form(form)
    try:
        ob = m.filter_sequences(k["pred_bad"], k["off"], eps=k["eps"], target=k["tgt"], want=want)
        ot = m.filter_sequences(k["pred"], k["off"], eps=k["eps"], target=k["tgt"], want=want)
    finally:
        m.set_seq_form(models.VAE.SEQ_FORM_DEFAULT)
    rb = so.filter(P, shape, k["pred_bad"], k["off"], k["eps"], target=k["tgt"])
    rt = so.filter(P, shape, k["pred"], k["off"], k["eps"], target=k["tgt"])
    nc.check_rows(rb["ref"], rt["ref"], k["mask"], "oracle ref")
    nc.check_rows(ob["ref"].cpu().numpy(), ot["ref"].cpu().numpy(), k["mask"], "ref")
    nc.check_rows(ob["frame_err"][:, 1].cpu().numpy(), ot["frame_err"][:, 1].cpu().numpy(), k["mask"], "err_ref")
    nc.check_rows(ob["seq_err"][:, 1].cpu().numpy(), ot["seq_err"][:, 1].cpu().numpy(), k["seq_mask"], "seq_err")
    vae_close(ot["ref"].cpu().numpy(), rt["ref"], "ref")
    vae_close(ot["frame_err"].cpu().numpy(), rt["frame_err"], "frame_err")
    np.testing.assert_allclose(ot["seq_err"].cpu().numpy(), rt["seq_err"], rtol=1e-5, atol=0)


def _vae_fresh(name, form=0):
    shape = nc.VAE_SHAPES[name]
    m = models.VAE(shape[0], shape[2], shape[1], shape[3], shape[4], max_batch=64, seed=1)
    m.set_weights(nc.vae_params(shape, 8))
    m.set_form(form)
    return m


def _vae_state_nan(m):
    mm, vv = m.slots()
    w = dict(zip([n for n, _, _ in m.param_table], m.get_weights()))
    return {tag: {n: np.isnan(a) for n, a in part.items()} for tag, part in (("w", w), ("m", mm), ("v", vv))}


@pytest.mark.parametrize("where", ["x", "t"])
def test_vae_gradients_and_adam_narrow(where):
    """compute_gradients + adam_apply at the narrow shape, B 17, one NaN in x[16] (or in t alone):
    the loss vector, every gradient element and, after Adam, every weight and both slots are NaN
    where the oracle's are -- everywhere."""
    k = nc.vae_case("default", 17, [16], seed=17)
    shape = k["shape"]
    P = nc.vae_params(shape, 8)
    x, t = (k["x_bad"], k["t"]) if where == "x" else (k["x"], k["t"].copy())
    if where == "t":
        t[3, 4] = np.nan
    c = vo.forward(P, shape, x, k["eps"])
    ref_loss = vo.loss3(vo.row_terms(c, t), nc.VAE_FACTORS)
    g_ref, _ = vo.backward(P, shape, c, t, nc.VAE_FACTORS)
    assert all(nc.all_nan(v) for v in g_ref.values())
    m = _vae_fresh("default")
    loss = m.compute_gradients(x, t, nc.VAE_FACTORS, eps=k["eps"]).cpu().numpy()
    np.testing.assert_array_equal(np.isnan(loss), np.isnan(ref_loss))
    g = m.grads()
    for n, ref in g_ref.items():
        np.testing.assert_array_equal(np.isnan(g[n]), np.isnan(ref), err_msg=n)
    m.adam_apply(1e-3)
    torch.cuda.synchronize()
    for tag, part in _vae_state_nan(m).items():
        for n, isn in part.items():
            assert isn.all(), (tag, n, int(isn.sum()), isn.size)       # NaN gradient -> NaN m, v and weight
    m.close()


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("where", ["x", "t"])
def test_vae_train_step_wide(form, where):
    """train_step_device at edge264 (the wide dx pass and k_vae_wide_wgrad_adam), forms 0 and 1."""
    k = nc.vae_case("edge264", 17, [16], seed=17)
    shape = k["shape"]
    P = nc.vae_params(shape, 8)
    x, t = (k["x_bad"], k["t"]) if where == "x" else (k["x"], k["t"].copy())
    if where == "t":
        t[3, 4] = np.nan
    c = vo.forward(P, shape, x, k["eps"])
    ref_loss = vo.loss3(vo.row_terms(c, t), nc.VAE_FACTORS)
    g_ref, _ = vo.backward(P, shape, c, t, nc.VAE_FACTORS)
    assert all(nc.all_nan(v) for v in g_ref.values())
    m = _vae_fresh("edge264", form)
    loss = m.train_step_device(x, t, nc.VAE_FACTORS, 1e-3, eps=k["eps"]).cpu().numpy()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(np.isnan(loss), np.isnan(ref_loss))
    g = m.grads()
    for n, ref in g_ref.items():
        np.testing.assert_array_equal(np.isnan(g[n]), np.isnan(ref), err_msg=n)
    for tag, part in _vae_state_nan(m).items():
        for n, isn in part.items():
            assert isn.all(), (tag, n, int(isn.sum()), isn.size)
    m.close()


# ------------------------------------------------------------------------------------------------
# the lifter's training step
# ------------------------------------------------------------------------------------------------

def _train_case(bn, B, where="x"):
    cfg = ref_mlp.Cfg(linear_size=256, num_layers=2, residual=True, batch_norm=bn)
    rng = np.random.default_rng(300 + B)
    x = rng.standard_normal((B, 32)).astype(np.float32)
    t = rng.standard_normal((B, 48)).astype(np.float32)
    if where == "x":
        x[B - 1, 7] = np.nan
    else:
        t[0, 0] = np.nan
    return cfg, x, t


def _train_model(cfg, B, seed=9):
    st = ref_mlp.init_state(cfg, seed=4, bn_seed=5)
    m = linear_model.LinearModel(cfg.linear_size, cfg.num_layers, cfg.residual, cfg.batch_norm, False, B, 1e-3,
                                 "/tmp/p3d_test", seed=seed, max_batch=64)
    m.set_weights({**st.params, **st.moving})
    return st, m


def _check_trained(m, st, out, ref_out, loss, what, everywhere=True):
    """After one step on both sides: NaN masks of y, the moving statistics, the weights and both
    Adam slots equal the oracle's (`everywhere`: which are all NaN)."""
    assert np.isnan(loss), (what, loss)
    np.testing.assert_array_equal(np.isnan(out), np.isnan(ref_out), err_msg=what + " y")
    state = m.get_state()
    for kname_, v in st.moving.items():
        np.testing.assert_array_equal(np.isnan(state[kname_]), np.isnan(v), err_msg=what + " " + kname_)
    for name in m.trainable_names():
        np.testing.assert_array_equal(np.isnan(state[name]), np.isnan(st.params[name]), err_msg=what + " " + name)
        np.testing.assert_array_equal(np.isnan(state[name + "/Adam"]), np.isnan(st.m[name]), err_msg=what + " m " + name)
        np.testing.assert_array_equal(np.isnan(state[name + "/Adam_1"]), np.isnan(st.v[name]), err_msg=what + " v " + name)
        assert np.isnan(st.params[name]).any() and (np.isnan(st.params[name]).all() or not everywhere), name
    clean(m)


@pytest.mark.parametrize("B", [64, 17])
@pytest.mark.parametrize("bn", [True, False])
@pytest.mark.parametrize("split,xchg", [("1", "1"), ("1", "0"), ("0", "1")])
def test_train_step_forms(split, xchg, bn, B, monkeypatch):
    """LinearModel.step(isTraining=True) with one NaN element in x, keep 0.5, on the three BN-train
    forms of test_train_steps_track_oracle: the loss is NaN; y, every gradient, the BN moving
    statistics and, after Adam, the weights and both slots are NaN where ref_mlp.train_step's are
    (y: all rows with BN, the bad row without; everything else: everywhere)."""
    monkeypatch.setenv("P3D_TRAIN_SPLIT", split)
    monkeypatch.setenv("P3D_TRAIN_XCHG", xchg)
    cfg, x, t = _train_case(bn, B)
    # the gradients, from a model of their own (compute_gradients applies the BN UPDATE_OPS too)
    st, m = _train_model(cfg, B)
    loss, y = m.compute_gradients(x, t, 0.5, ctr=0)
    out, cache = ref_mlp.forward(st, x, True, 0.5, m.seed, 0, 0)
    rl, dy = ref_mlp.mse(out, t)
    grads = ref_mlp.backward(st, cache, dy)
    assert np.isnan(rl) and np.isnan(float(loss.item()))
    np.testing.assert_array_equal(np.isnan(y.cpu().numpy()), np.isnan(out))
    want_rows = np.ones(B, bool) if bn else np.arange(B) == B - 1
    np.testing.assert_array_equal(np.isnan(out).all(axis=1), want_rows)
    for name in m.trainable_names():
        g = m.grad(name).cpu().numpy()
        assert np.isnan(grads[name]).all(), name
        np.testing.assert_array_equal(np.isnan(g), np.isnan(grads[name]), err_msg=name)
    clean(m)
    m.close()
    # the whole step
    st, m = _train_model(cfg, B)
    loss, _, _, out = m.step(None, x.astype(np.float64), t.astype(np.float64), 0.5, isTraining=True)
    rl, ro = ref_mlp.train_step(st, x, t, 0.5, 1e-3, seed=m.seed, ctr=0)
    assert np.isnan(rl)
    _check_trained(m, st, out, ro, loss, "step")
    m.close()


@pytest.mark.parametrize("B", [64, 17])
@pytest.mark.parametrize("bn", [True, False])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("where", ["x", "t"])
def test_train_step_fused_and_unfused(where, fused, bn, B, monkeypatch):
    """The fused step (P3D_FUSE_ADAM=1: Adam inside the gradient kernels) and the unfused one
    (p3d_train_fwd_bwd + p3d_adam_step_decay) of test_fused_train_step_bit_identical_to_unfused.
    where = t: the NaN sits in the target alone, at t[0, 0] -- y stays finite, the loss is NaN, the
    output layer's gradient is NaN in output column 0 only and everything below it throughout (the
    ReLU backward is a product: a NaN gradient under a dead unit stays NaN)."""
    monkeypatch.setenv("P3D_FUSE_ADAM", "1")
    cfg, x, t = _train_case(bn, B, where)
    st, m = _train_model(cfg, B)
    xd, td = dev(x), dev(t)
    y = torch.empty((B, 48), device="cuda")
    if fused:
        m.train_step_device(xd, td, 0.5, out=y)
    else:
        _p3d.check(_p3d.lib().p3d_train_fwd_bwd(m._h, xd.data_ptr(), td.data_ptr(), B, y.data_ptr(), 0.5, m.seed, 0,
                                                 m._loss_dev.data_ptr(), m.stream()), "fb")
        _p3d.check(_p3d.lib().p3d_adam_step_decay(m._h, m.lr0, 100000.0, 0.96, m.stream()), "adam")
    torch.cuda.synchronize()
    rl, ro = ref_mlp.train_step(st, x, t, 0.5, 1e-3, seed=m.seed, ctr=0)
    assert np.isnan(rl)
    if where == "t":
        assert not np.isnan(ro).any() and not np.isnan(st.params["linear_model/w4"][:, 1:]).any()
    _check_trained(m, st, y.cpu().numpy(), ro, float(m._loss_dev.item()), "fused" if fused else "unfused", where == "x")
    m.close()
