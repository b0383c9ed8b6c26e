"""GPU tests of the VAE filter averaged over K posterior samples inside one launch
(csrc/p3d_vae_mc.h: k_vae_fwd_mc, k_vae_fwd_mc_cat, k_vae_seq4_mc; VAE.forward_device and
VAE.filter_sequences with samples=K; the drivers' --filter_samples).

Bounds.  Against the composition -- K p3d_vae_forward launches and the fold written with torch
elementwise operations, or the per-frame host loop for sequences -- bit for bit.  Against the
float64 oracle (tests/vae_mc_oracle.py): the mean within the project's forward bound
2e-5 + 2e-5 |ref|, the variance within the bound that propagates from it,
c_{K-1} sum_k (4 b |d_k| + 4 b^2) + 1e-5 var_ref (vae_mc_oracle.var_bound).
"""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import _p3d
import vae_mc_oracle as mo
import vae_oracle as vo
from _p3d import ptr
from top_vae_3d_pose import models

pytestmark = pytest.mark.gpu

SHAPES = {
    "default": vo.DEFAULT_SHAPE,                  # 48 -> 40 -> 32 -> 24 -> 32 -> 40 -> 48
    "edge": (48, (8,), 8, (24,), 48),             # widths 8 mod 16: the padded MFMA tiles
    "edge264": (264, (8,), 8, (24,), 48),         # the wide form: k_vae_wide_fwd, then the core over h0
    "in80": (80, (40, 32), 24, (32, 40), 48),     # [x2d | out_3d]
    "in144": (144, (40, 32), 24, (32, 40), 48),   # the sequence filter's two shapes (tests/test_gpu_vae_seq.py)
    "edge96": (96, (8,), 8, (24,), 48),
}
FWD_SHAPES = ("default", "edge", "edge264")
SEQ_SHAPES = ("in144", "edge96")
BATCHES = (1, 17, 65)        # one row; a ragged second tile; a second 64-row block and a wave with no tile
KS = (1, 2, 5, 16)
SEQ_KS = (1, 3)
# tests/test_gpu_vae_seq.py's 33 sequences: three tiles, the last a single row; ragged, max 64, one empty
LENS = [1, 2, 3, 64, 5, 0, 17, 33, 8, 16, 15, 4, 63, 9, 2, 31,
        7, 1, 12, 40, 3, 6, 20, 11, 2, 5, 48, 10, 3, 14, 1, 9,
        13]


def rand_params(shape, seed):
    P = vo.init_params(shape, seed)
    rng = np.random.default_rng(seed + 1)
    for k in P:
        if k.endswith("/bias"):
            P[k] = (0.1 * rng.standard_normal(P[k].shape)).astype(np.float32)
    return P


def fwd_bound(ref):
    return 2e-5 + 2e-5 * np.abs(np.asarray(ref, np.float64))


def ck(k):
    """c_k as the Python float torch multiplies by."""
    return float(np.float32(1.0 / (k + 1)))


def torch_fold(ys):
    """The fold over a list of K device tensors with torch elementwise operations, one rounding each."""
    m = ys[0].clone()
    M = torch.zeros_like(m)
    for k in range(1, len(ys)):
        d = ys[k] - m
        dc = d * ck(k)
        m = m + dc
        d2 = ys[k] - m
        M = M + d * d2
    return m, M * ck(len(ys) - 1)


_models, _cases, _seq_cases, _frame_paths = {}, {}, {}, {}


def model_of(name):
    if name not in _models:
        shape = SHAPES[name]
        m = models.VAE(shape[0], shape[2], shape[1], shape[3], shape[4], max_batch=1024, seed=5)
        m.set_weights(rand_params(shape, 3))
        _models[name] = m
    return _models[name]


def case_of(name, B):
    """Inputs on the device, 16 draws, and the K plain forwards of each draw (computed once)."""
    if (name, B) not in _cases:
        shape, m = SHAPES[name], model_of(name)
        rng = np.random.default_rng(1000 * B + len(name))
        x = rng.standard_normal((B, shape[0])).astype(np.float32)
        eps = rng.standard_normal((max(KS), B, shape[2])).astype(np.float32)
        xd, ed = torch.from_numpy(x).cuda(), torch.from_numpy(eps).cuda()
        plain = [m.forward_device(xd, eps=ed[k], want=("y", "mean", "log_var")) for k in range(max(KS))]
        _cases[(name, B)] = dict(x=x, eps=eps, xd=xd, ed=ed, plain=plain)
    return _cases[(name, B)]


# ------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", FWD_SHAPES)
def test_forward_bit_equal_to_the_composition(name, B, K):
    m, k = model_of(name), case_of(name, B)
    o = m.forward_device(k["xd"], eps=k["ed"][:K], want=("y", "y_var", "mean", "log_var"), samples=K)
    y, var = torch_fold([p["y"] for p in k["plain"][:K]])
    assert torch.equal(o["y"], y)
    assert torch.equal(o["y_var"], var)
    assert torch.equal(o["mean"], k["plain"][0]["mean"]) and torch.equal(o["log_var"], k["plain"][0]["log_var"])
    if K == 1:
        assert torch.equal(o["y"], k["plain"][0]["y"]) and not o["y_var"].any()
    else:
        assert (o["y_var"] > 0).any()
    # only what was asked for is written: y alone is the same y
    assert torch.equal(m.forward_device(k["xd"], eps=k["ed"][:K], samples=K)["y"], o["y"])


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", FWD_SHAPES)
def test_forward_vs_float64_oracle(name, B, K):
    m, k = model_of(name), case_of(name, B)
    o = m.forward_device(k["xd"], eps=k["ed"][:K], want=("y", "y_var", "mean", "log_var"), samples=K)
    want = mo.forward(rand_params(SHAPES[name], 3), SHAPES[name], k["x"], k["eps"][:K])
    y, var = o["y"].double().cpu().numpy(), o["y_var"].double().cpu().numpy()
    r_y = np.abs(y - want["y"]) / fwd_bound(want["y"])
    b = fwd_bound(want["ys"]).max(axis=0)
    vb = mo.var_bound(want["ys"], b)
    r_v = np.abs(var - want["y_var"]) / vb
    print("%s B %d K %d: worst ratio to the bound: y %.3g, y_var %.3g" % (name, B, K, r_y.max(), r_v.max()))
    assert r_y.max() <= 1.0
    assert r_v.max() <= 1.0
    for key in ("mean", "log_var"):
        assert (np.abs(o[key].double().cpu().numpy() - want[key]) <= fwd_bound(want[key])).all(), key


@pytest.mark.parametrize("name", FWD_SHAPES)
def test_internal_stream_is_the_eps_kernel_at_ctr_plus_k(name):
    m, k = model_of(name), case_of(name, 65)
    K, c = 5, 21
    a = m.forward_device(k["xd"], eps=None, ctr=c, want=("y", "y_var"), samples=K)
    eps = torch.stack([m.eps_device(65, ctr=c + j) for j in range(K)])
    b = m.forward_device(k["xd"], eps=eps, want=("y", "y_var"), samples=K)
    assert torch.equal(a["y"], b["y"]) and torch.equal(a["y_var"], b["y_var"])
    # draw j is the plain forward's own draw at counter c + j
    plain = [m.forward_device(k["xd"], eps=None, ctr=c + j)["y"] for j in range(K)]
    y, var = torch_fold(plain)
    assert torch.equal(a["y"], y) and torch.equal(a["y_var"], var)
    n = m.forward_device(k["xd"], eps=None, ctr=c + 1, want=("y", "y_var"), samples=K)
    assert not torch.equal(a["y"], n["y"]) and not torch.equal(a["y_var"], n["y_var"])


@pytest.mark.parametrize("K", (1, 5))
def test_segments_equal_the_materialised_concatenation(K):
    rng = np.random.default_rng(4)
    B = 65
    # [x2d | out_3d], in = 80: the narrow _cat kernel
    m = model_of("in80")
    x2d = torch.from_numpy(rng.standard_normal((B, 32)).astype(np.float32)).cuda()
    o3d = torch.from_numpy(rng.standard_normal((B, 48)).astype(np.float32)).cuda()
    eps = torch.from_numpy(rng.standard_normal((K, B, 24)).astype(np.float32)).cuda()
    want = ("y", "y_var", "mean", "log_var")
    a = m.forward_device([x2d, o3d], eps=eps, want=want, samples=K)
    b = m.forward_device(torch.cat([x2d, o3d], dim=1), eps=eps, want=want, samples=K)
    for key in want:
        assert torch.equal(a[key], b[key]), key
    # a (table, idx) segment on the wide form
    w = model_of("edge264")
    head = torch.from_numpy(rng.standard_normal((B, 8)).astype(np.float32)).cuda()
    table = torch.from_numpy(rng.standard_normal((40, 256)).astype(np.float32)).cuda()
    idx = torch.from_numpy(rng.integers(0, 40, size=B)).cuda()
    eps = torch.from_numpy(rng.standard_normal((K, B, 8)).astype(np.float32)).cuda()
    a = w.forward_device([head, (table, idx)], eps=eps, want=want, samples=K)
    b = w.forward_device(torch.cat([head, table[idx]], dim=1), eps=eps, want=want, samples=K)
    for key in want:
        assert torch.equal(a[key], b[key]), key
    assert K == 1 or (a["y_var"] > 0).any()


@pytest.mark.parametrize("name", FWD_SHAPES)
def test_a_nan_input_row_stays_in_its_row(name):
    m, k = model_of(name), case_of(name, 17)
    K, bad = 5, 3
    clean = m.forward_device(k["xd"], eps=k["ed"][:K], want=("y", "y_var"), samples=K)
    x = k["xd"].clone()
    x[bad] = float("nan")
    o = m.forward_device(x, eps=k["ed"][:K], want=("y", "y_var"), samples=K)
    keep = torch.arange(17, device="cuda") != bad
    for key in ("y", "y_var"):
        assert torch.isnan(o[key][bad]).all(), key
        assert torch.equal(o[key][keep], clean[key][keep]), key


def test_forward_graph_replays():
    m, k = model_of("default"), case_of("default", 65)
    K = 5
    x = k["xd"].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.forward_device(x, eps=k["ed"][:K], want=("y", "y_var"), samples=K)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        o = m.forward_device(x, eps=k["ed"][:K], want=("y", "y_var"), samples=K)
    eager = m.forward_device(k["xd"], eps=k["ed"][:K], want=("y", "y_var"), samples=K)
    for _ in range(2):
        o["y"].fill_(float("nan"))
        o["y_var"].fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o["y"], eager["y"]) and torch.equal(o["y_var"], eager["y_var"])
    x.mul_(0.5)      # the graph reads its inputs anew at every replay
    g.replay()
    torch.cuda.synchronize()
    half = m.forward_device(x, eps=k["ed"][:K], samples=K)["y"]
    assert torch.equal(o["y"], half) and not torch.equal(half, eager["y"])


def test_python_refusals_and_the_bones_filter():
    m, k = model_of("default"), case_of("default", 17)
    with pytest.raises(ValueError):
        m.forward_device(k["xd"], samples=2, want=("y", "z"))
    with pytest.raises(ValueError):
        m.forward_device(k["xd"], samples=2, target=k["xd"])
    with pytest.raises(ValueError):
        m.forward_device(k["xd"], samples=2, eps=k["ed"][0])             # eps must be [K, B, latent]
    with pytest.raises(ValueError):
        m.forward_device(k["xd"], samples=3, eps=k["ed"][:2])
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError):
            m.forward_device(k["xd"], samples=bad)
    with pytest.raises(ValueError):
        m.forward_device(k["xd"], samples=2, want=("y", "row_terms"))
    # calling the model: the mean of K samples at counters calls + 1 .. calls + K
    calls = m._calls
    y = m(k["xd"], samples=4)
    assert m._calls == calls + 4
    assert torch.equal(y, m.forward_device(k["xd"], ctr=calls + 1, samples=4)["y"])
    # a bones filter: direction cosines do not average
    b = models.VAEBones(64, 8, (24,), (24,), max_batch=64, seed=1)
    x = torch.zeros((4, 64), device="cuda")
    with pytest.raises(NotImplementedError):
        b.forward_device(x, samples=2)
    with pytest.raises(NotImplementedError):
        b(x, samples=2)
    y = torch.empty((4, 64), device="cuda")
    lib = _p3d.lib()
    assert lib.p3d_vae_forward_mc(b._h, ptr(x), 4, 2, None, 0, ptr(y), None, None, None, None) == _p3d.P3D_ERR_ARG
    assert b"direction cosines do not average" in lib.p3d_last_error()
    off = torch.tensor([0, 4], device="cuda")
    assert lib.p3d_vae_seq_filter_mc(b._h, ptr(x), ptr(off), 1, 4, 2, None, 0, 0, None, None, None, ptr(y), None, None,
                                     None, None) == _p3d.P3D_ERR_ARG
    assert b"direction cosines do not average" in lib.p3d_last_error()
    b.close()


def test_lifter_plus_filter_models_pass_samples_on():
    """Pose3DVae and Pose3DVaeCat (use_2d: the _cat kernel) with samples=K equal the filter's own call on
    the lifter's output at the same counters; Pose3DVaeBones refuses."""
    import linear_model
    from oracle import ref_mlp
    cfg = ref_mlp.Cfg(linear_size=128, num_layers=1, residual=True, batch_norm=True)
    st = ref_mlp.init_state(cfg, seed=5, bn_seed=6)
    lifter = linear_model.LinearModel(128, 1, True, True, False, 64, 1e-3, "/tmp/p3d_vae_mc_pose", seed=7)
    lifter.set_weights({**st.params, **st.moving})
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((70, 32)).astype(np.float32)).cuda()
    K = 3
    pv = models.Pose3DVae(24, [40, 32], [32, 40], pose3d=lifter, max_batch=256, seed=3)
    calls = pv.vae._calls
    out_3d, out_vae = pv(x, training=False, samples=K)
    assert pv.vae._calls == calls + K
    assert torch.equal(out_vae, pv.vae.forward_device(out_3d, ctr=calls + 1, samples=K)["y"])
    eps = torch.randn((K, 70, 24), device="cuda")
    assert torch.equal(pv(x, eps=eps, samples=K)[1], pv.vae.forward_device(out_3d, eps=eps, samples=K)["y"])
    pv.close()
    pc = models.Pose3DVaeCat(24, [40, 32], [32, 40], use_2d=True, pose3d=lifter, max_batch=256, seed=3)
    calls = pc.vae._calls
    out_3d, out_vae = pc(x, training=False, samples=K)
    assert pc.vae._calls == calls + K
    assert torch.equal(out_vae, pc.vae.forward_device(torch.cat([x, out_3d], dim=1), ctr=calls + 1, samples=K)["y"])
    pc.close()
    pb = models.Pose3DVaeBones(8, [24], [24], use_2d=True, pose3d=lifter, max_batch=256, seed=3)
    with pytest.raises(NotImplementedError):
        pb(x, samples=K)
    pb.close()
    lifter.close()


# ---------------------------------------------------------------------------------------- sequences
def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def seq_case_of(name):
    if name not in _seq_cases:
        shape = SHAPES[name]
        out, lat = shape[4], shape[2]
        rng = np.random.default_rng(len(name))
        off = offsets(LENS)
        N = int(off[-1])
        pred = torch.from_numpy(rng.standard_normal((N, out)).astype(np.float32)).cuda()
        eps = torch.from_numpy(rng.standard_normal((max(SEQ_KS), N, lat)).astype(np.float32)).cuda()
        tgt = torch.from_numpy(rng.standard_normal((N, out)).astype(np.float32)).cuda()
        _seq_cases[name] = dict(off=off, N=N, pred=pred, eps=eps, tgt=tgt)
    return _seq_cases[name]


def row_err(t, y):
    """mean_out (t - y)^2 per row in the kernels' association: four chains over the columns q, q + 4,
    ..., summed (p0 + p1) + (p2 + p3), then one correctly rounded division (tensor by tensor)."""
    out = t.shape[1]
    df = t - y
    sq = df * df
    p = []
    for q in range(4):
        acc = torch.zeros_like(sq[:, 0])
        for c in range(q, out, 4):
            acc = acc + sq[:, c]
        p.append(acc)
    s = (p[0] + p[1]) + (p[2] + p[3])
    return s / torch.full_like(s, float(out))


def frame_path_of(name, K):
    """The per-frame path: the host loop over frames of tests/test_gpu_vae_seq.py with
    forward_device(x, eps=eps[:, g], samples=K) in place of the plain forward and y fed back."""
    if (name, K) in _frame_paths:
        return _frame_paths[(name, K)]
    shape, m, k = SHAPES[name], model_of(name), seq_case_of(name)
    out, L, N = shape[4], shape[0] // shape[4], k["N"]
    pred, eps, tgt = k["pred"], k["eps"][:K], k["tgt"]
    lens = torch.tensor(LENS, device="cuda")
    offd = torch.from_numpy(k["off"][:-1]).cuda()
    buf = pred[offd.clamp(max=N - 1)].repeat(1, L)
    ref = torch.full((N, out), float("nan"), device="cuda")
    var = torch.full((N, out), float("nan"), device="cuda")
    err = torch.full((N,), float("nan"), device="cuda")
    for f in range(max(LENS)):
        rows = torch.nonzero(lens > f).flatten()
        g = offd[rows] + f
        x = torch.cat([buf[rows, out:], pred[g]], dim=1)
        o = m.forward_device(x, eps=eps[:, g].contiguous(), want=("y", "y_var"), samples=K)
        x[:, (L - 1) * out:] = o["y"]
        buf[rows] = x
        ref[g], var[g], err[g] = o["y"], o["y_var"], row_err(tgt[g], o["y"])
    assert not torch.isnan(ref).any()
    _frame_paths[(name, K)] = dict(ref=ref, ref_var=var, err_ref=err)
    return _frame_paths[(name, K)]


ALL = ("ref", "ref_var", "frame_err", "seq_err")


@pytest.mark.parametrize("K", SEQ_KS)
@pytest.mark.parametrize("name", SEQ_SHAPES)
def test_sequences_bit_equal_to_the_per_frame_path(name, K):
    m, k, w = model_of(name), seq_case_of(name), frame_path_of(name, K)
    o = m.filter_sequences(k["pred"], k["off"], eps=k["eps"][:K], target=k["tgt"], want=ALL, samples=K)
    assert torch.equal(o["ref"], w["ref"])
    assert torch.equal(o["ref_var"], w["ref_var"])
    assert torch.equal(o["frame_err"][:, 1], w["err_ref"])
    fe = o["frame_err"].double().cpu().numpy()
    want = np.array([[sum(fe[a:b, j]) for j in range(2)] for a, b in zip(k["off"][:-1], k["off"][1:])])
    np.testing.assert_allclose(o["seq_err"].cpu().numpy(), want, rtol=1e-15, atol=0)
    # ref alone, without a target, is the same ref
    assert torch.equal(m.filter_sequences(k["pred"], k["off"], eps=k["eps"][:K], samples=K)["ref"], w["ref"])
    if K == 1:      # the plain sequence filter's bits, ref and both errors
        p = m.filter_sequences(k["pred"], k["off"], eps=k["eps"][0], target=k["tgt"], want=("ref", "frame_err", "seq_err"))
        assert torch.equal(o["ref"], p["ref"]) and torch.equal(o["frame_err"], p["frame_err"])
        assert torch.equal(o["seq_err"], p["seq_err"]) and not o["ref_var"].any()
    else:
        assert (o["ref_var"] > 0).any()


@pytest.mark.parametrize("at", [1, 2, 7])
@pytest.mark.parametrize("name", SEQ_SHAPES)
def test_chunked_calls_equal_one_call(name, at):
    import vae_seq_oracle as so
    m, k, K = model_of(name), seq_case_of(name), 3
    i1, o1, i2, o2 = so.split(k["off"], at)
    d1, d2 = torch.from_numpy(i1).cuda(), torch.from_numpy(i2).cuda()
    eps = k["eps"][:K]
    whole = m.filter_sequences(k["pred"], k["off"], eps=eps, target=k["tgt"], want=ALL, samples=K)
    st = m.new_seq_state(len(LENS))
    a = m.filter_sequences(k["pred"][d1], o1, eps=eps[:, d1], target=k["tgt"][d1], state=st, want=ALL, samples=K)
    started = st[1].cpu().numpy().copy()
    b = m.filter_sequences(k["pred"][d2], o2, eps=eps[:, d2], target=k["tgt"][d2], state=st, want=ALL, samples=K)
    assert started.tolist() == [int(n > 0) for n in LENS]
    for key in ("ref", "ref_var", "frame_err"):
        assert torch.equal(a[key], whole[key][d1]) and torch.equal(b[key], whole[key][d2]), key
    np.testing.assert_allclose((a["seq_err"] + b["seq_err"]).cpu().numpy(), whole["seq_err"].cpu().numpy(),
                               rtol=1e-12, atol=0)
    assert not st[0][LENS.index(0)].any()


@pytest.mark.parametrize("name", SEQ_SHAPES)
def test_order_independence(name):
    m, k, K = model_of(name), seq_case_of(name), 3
    eps = k["eps"][:K]
    want = ("ref", "ref_var", "frame_err")
    whole = m.filter_sequences(k["pred"], k["off"], eps=eps, target=k["tgt"], want=want, samples=K)
    perm = np.random.default_rng(9).permutation(len(LENS))
    idx = torch.from_numpy(np.concatenate([np.arange(k["off"][s], k["off"][s + 1]) for s in perm])).cuda()
    o = m.filter_sequences(k["pred"][idx], offsets([LENS[s] for s in perm]), eps=eps[:, idx], target=k["tgt"][idx],
                           want=want, samples=K)
    for key in want:
        assert torch.equal(o[key], whole[key][idx]), key


@pytest.mark.parametrize("name", SEQ_SHAPES)
def test_internal_sequence_stream_is_the_eps_kernel(name):
    m, k, K = model_of(name), seq_case_of(name), 3
    c, r = 11, 1000
    a = m.filter_sequences(k["pred"], k["off"], eps=None, ctr=c, eps_row0=r, want=("ref", "ref_var"), samples=K)
    eps = torch.stack([m.eps_device(k["N"], ctr=c + j, row0=r) for j in range(K)])
    b = m.filter_sequences(k["pred"], k["off"], eps=eps, want=("ref", "ref_var"), samples=K)
    assert torch.equal(a["ref"], b["ref"]) and torch.equal(a["ref_var"], b["ref_var"])
    n = m.filter_sequences(k["pred"], k["off"], eps=None, ctr=c + 1, eps_row0=r, samples=K)["ref"]
    assert not torch.equal(a["ref"], n)
    # a fresh counter advances the call counter by K
    calls = m._calls
    m.filter_sequences(k["pred"], k["off"], samples=K)
    assert m._calls == calls + K


def test_sequences_vs_float64_oracle():
    name, shape, K = "in144", SHAPES["in144"], 3
    m = model_of(name)
    S, T = 20, 64
    rng = np.random.default_rng(21)
    off = np.arange(S + 1, dtype=np.int64) * T
    pred = rng.standard_normal((S * T, 48)).astype(np.float32)
    eps = rng.standard_normal((K, S * T, 24)).astype(np.float32)
    tgt = rng.standard_normal((S * T, 48)).astype(np.float32)
    want = mo.filter(rand_params(shape, 3), shape, pred, off, eps, target=tgt)
    o = m.filter_sequences(pred, off, eps=eps, target=tgt, want=ALL, samples=K)
    ref, var = o["ref"].double().cpu().numpy(), o["ref_var"].double().cpu().numpy()
    r_y = np.abs(ref - want["ref"]) / fwd_bound(want["ref"])
    vb = mo.var_bound(want["ys"], fwd_bound(want["ys"]).max(axis=0))
    r_v = np.abs(var - want["ref_var"]) / vb
    fe = o["frame_err"].double().cpu().numpy()
    r_e = np.abs(fe - want["frame_err"]) / fwd_bound(want["frame_err"])
    print("free-running K %d: worst ratio to the bound: ref %.3g, ref_var %.3g, frame_err %.3g"
          % (K, r_y.max(), r_v.max(), r_e.max()))
    assert r_y.max() <= 1.0
    assert r_v.max() <= 1.0
    assert r_e.max() <= 1.0
    np.testing.assert_allclose(o["seq_err"].cpu().numpy(), want["seq_err"], rtol=1e-5, atol=0)


def test_sequence_refusals_and_graph_replay():
    m, k = model_of("in144"), seq_case_of("in144")
    K = 3
    eps = k["eps"][:K]
    with pytest.raises(ValueError):
        m.filter_sequences(k["pred"], k["off"], eps=eps[0], samples=K)            # eps must be [K, N, latent]
    with pytest.raises(ValueError):
        m.filter_sequences(k["pred"], k["off"], eps=eps, want=("ref", "ref_var"))  # ref_var needs samples
    with pytest.raises(ValueError):
        m.filter_sequences(k["pred"], k["off"], eps=eps, samples=K, want=("ref", "frame_err"))   # no target
    with pytest.raises(ValueError):
        m.filter_sequences(k["pred"], k["off"], samples=65)
    odd = model_of("in80")                                                       # in is no multiple of out
    with pytest.raises(ValueError):
        odd.filter_sequences(k["pred"], k["off"], samples=K)
    lib = _p3d.lib()
    off = torch.from_numpy(k["off"]).cuda()
    out = torch.empty_like(k["pred"])
    assert lib.p3d_vae_seq_filter_mc(odd._h, ptr(k["pred"]), ptr(off), 33, k["N"], K, None, 0, 0, None, None, None,
                                     ptr(out), None, None, None, None) == _p3d.P3D_ERR_ARG
    fe = torch.empty((k["N"], 2), device="cuda")
    assert lib.p3d_vae_seq_filter_mc(m._h, ptr(k["pred"]), ptr(off), 33, k["N"], K, None, 0, 0, None, None, None,
                                     ptr(out), None, ptr(fe), None, None) == _p3d.P3D_ERR_ARG
    # a captured call replays to the same bits
    pred = k["pred"].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.filter_sequences(pred, off, eps=eps, target=k["tgt"], want=ALL, samples=K)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        o = m.filter_sequences(pred, off, eps=eps, target=k["tgt"], want=ALL, samples=K)
    eager = m.filter_sequences(k["pred"], k["off"], eps=eps, target=k["tgt"], want=ALL, samples=K)
    for _ in range(2):
        o["ref"].fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for key in ALL:
            assert torch.equal(o[key], eager[key]), key


# ------------------------------------------------------------------------------------------- driver
def test_driver_filter_samples(tmp_path, capsys):
    """3d_pose_vae_filter_kin.py on synthetic H3.6M archives with a tiny lifter, one epoch:
    --filter_samples 1 reproduces the run without the flag exactly (training history, weights and
    the evaluation); --evaluate --filter_samples 3 prints the per-key variance line and its ref is
    filter_sequences(..., samples=3) on the same inputs."""
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "golden"))
    from synth_cameras import write_h36m_archives
    tree, camsp = str(tmp_path / "h36m.npz"), str(tmp_path / "cameras.npz")
    write_h36m_archives(tree, camsp, np.random.default_rng(31), ["Walking"], frames=120, sh=False)
    spec = importlib.util.spec_from_file_location(
        "pose_vae_filter_kin_mc", os.path.join(os.path.dirname(here), "3d-pose-baseline_amd", "3d_pose_vae_filter_kin.py"))
    kin = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kin)
    cfg = tmp_path / "train.yml"
    cfg.write_text("train:\n  step_log: 2000\n  learning_rate: 0.0001\n  likelihood_factor: 100.0\n"
                   "  kcs_factor: 0.02\n  dkl_factor: 1.0\n")

    def argv(d, *more):
        return ["--camera_frame", "--action", "Walking", "--data_dir", tree, "--cameras_path", camsp,
                "--linear_size", "128", "--num_layers", "1", "--residual", "--batch_norm", "--cfg_file", str(cfg),
                "--train_dir", str(tmp_path / d), "--epochs", "1", "--seed", "3"] + list(more)

    def train(d, *more):
        np.random.seed(5)
        model, hist = kin.train(argv(d, *more), read_from_config=True)
        w = model.get_weights()
        model.close()
        return hist, w, kin.weights_path() + ".npz"

    h0, w0, saved = train("a")
    h1, w1, _ = train("b", "--filter_samples", "1")
    for key in h0:
        np.testing.assert_array_equal(np.asarray(h0[key]), np.asarray(h1[key]), err_msg=key)
    for a, b in zip(w0, w1):
        np.testing.assert_array_equal(a, b)
    h3, w3, _ = train("c", "--filter_samples", "3")       # the test block on the mean of three samples
    for a, b in zip(w0, w3):
        np.testing.assert_array_equal(a, b)                # (training itself does not move)
    assert np.isfinite(h3["pred_error"]).all() and h3["pred_error"] != h0["pred_error"]

    def evaluate(*more):
        capsys.readouterr()
        res = kin.evaluate(argv("a", "--evaluate", "--vae_weights", saved, *more), read_from_config=True)
        return res, capsys.readouterr().out

    r0, out0 = evaluate()
    r1, out1 = evaluate("--filter_samples", "1")
    assert out0 == out1 and "sample variance" not in out0
    assert torch.equal(r0["ref"], r1["ref"]) and torch.equal(r0["frame_err"], r1["frame_err"])
    assert r0["per_key"] == r1["per_key"] and r0["overall"] == r1["overall"] and "ref_var" not in r1
    r3, out3 = evaluate("--filter_samples", "3")
    assert out3.count("VAE sample variance (3 samples):") == len(r3["keys"]) > 0
    vae = r3["vae"]
    o = vae.filter_sequences(r3["pred"], r3["seq_off"], ctr=r3["eps_ctr"], eps_row0=0, target=r3["target"],
                             want=ALL, samples=3)
    assert torch.equal(r3["ref"], o["ref"]) and torch.equal(r3["ref_var"], o["ref_var"])
    assert torch.equal(r3["frame_err"], o["frame_err"])
    off = r3["seq_off"]
    for i, key in enumerate(r3["keys"]):
        lo, hi = int(off[i]), int(off[i + 1])
        assert r3["per_key_var"][key] == float(o["ref_var"][lo:hi].double().mean()) > 0
        assert ("VAE sample variance (3 samples): %s" % r3["per_key_var"][key]) in out3
    assert not torch.equal(r3["ref"], r0["ref"])
    for r in (r0, r1, r3):
        r["vae"].close()
        r["pose3d"].close()
