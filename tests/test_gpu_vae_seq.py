"""GPU tests of the temporal filter's recurrence over whole sequences (csrc/p3d_vae_seq.h,
VAE.filter_sequences) against the per-frame path (p3d_vae_forward) and tests/vae_seq_oracle.py.

Bounds: against the per-frame path, other sequence orders, chunked calls, the other launch form and
the integer model: bit for bit.  Against the free-running float64 oracle: the project's forward
bound 2e-5 + 2e-5 |ref| on ref and frame_err (the float32 oracle drifts from float64 by <= 5e-7 over
the 64 frames: the map contracts for these weights), seq_err 1e-5 relative.
"""
import ctypes

import numpy as np
import pytest
import torch

import _p3d
import vae_oracle as vo
import vae_seq_oracle as so
from _p3d import ptr
from top_vae_3d_pose import models

pytestmark = pytest.mark.gpu

SHAPES = {
    "in144": (144, (40, 32), 24, (32, 40), 48),
    "edge96": (96, (8,), 8, (24,), 48),           # seq_len 2, widths 8 mod 16
}
# 33 sequences: three tiles, the last a single row; ragged, max 64, one empty
LENS = [1, 2, 3, 64, 5, 0, 17, 33, 8, 16, 15, 4, 63, 9, 2, 31,
        7, 1, 12, 40, 3, 6, 20, 11, 2, 5, 48, 10, 3, 14, 1, 9,
        13]
assert len(LENS) == 33 and max(LENS) == 64 and 0 in LENS


def rand_params(shape, seed):
    P = vo.init_params(shape, seed)
    rng = np.random.default_rng(seed + 1)
    for k in P:
        if k.endswith("/bias"):
            P[k] = (0.1 * rng.standard_normal(P[k].shape)).astype(np.float32)
    return P


def close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref) - (2e-5 + 2e-5 * np.abs(ref))
    assert err.max() <= 0, (what, float(np.abs(got - ref).max()))


_models, _cases = {}, {}


def model_of(name):
    if name not in _models:
        shape = SHAPES[name]
        m = models.VAE(shape[0], shape[2], shape[1], shape[3], shape[4], max_batch=1024, seed=5)
        m.set_weights(rand_params(shape, 3))
        _models[name] = m
    return _models[name]


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def case_of(name):
    """The ragged case of a shape and, computed once, what the per-frame path gives for it: a host
    loop over frames that assembles the windows with torch ops and calls forward_device."""
    if name in _cases:
        return _cases[name]
    shape, m = SHAPES[name], model_of(name)
    out, lat, L = shape[4], shape[2], shape[0] // shape[4]
    rng = np.random.default_rng(len(name))
    off = offsets(LENS)
    N = int(off[-1])
    pred = torch.from_numpy(rng.standard_normal((N, out)).astype(np.float32)).cuda()
    eps = torch.from_numpy(rng.standard_normal((N, lat)).astype(np.float32)).cuda()
    tgt = torch.from_numpy(rng.standard_normal((N, out)).astype(np.float32)).cuda()
    lens = torch.tensor(LENS, device="cuda")
    offd = torch.from_numpy(off[:-1]).cuda()
    buf = pred[offd.clamp(max=N - 1)].repeat(1, L)          # [p0] * seq_len (rows of empty sequences: unused)
    ref = torch.full((N, out), float("nan"), device="cuda")
    err_ref = torch.full((N,), float("nan"), device="cuda")
    for f in range(max(LENS)):
        rows = torch.nonzero(lens > f).flatten()
        g = offd[rows] + f
        x = torch.cat([buf[rows, out:], pred[g]], dim=1)
        o = m.forward_device(x, eps=eps[g], target=tgt[g])
        x[:, (L - 1) * out:] = o["y"]
        buf[rows] = x
        ref[g] = o["y"]
        err_ref[g] = o["row_terms"][:, 0]
    assert not torch.isnan(ref).any()
    _cases[name] = dict(off=off, N=N, pred=pred, eps=eps, tgt=tgt, ref=ref, err_ref=err_ref)
    return _cases[name]


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", list(SHAPES))
def test_bit_equal_to_the_per_frame_path(name, form):
    m, k = model_of(name), case_of(name)
    m.set_seq_form(form)
    try:
        o = m.filter_sequences(k["pred"], k["off"], eps=k["eps"], target=k["tgt"], want=("ref", "frame_err", "seq_err"))
    finally:
        m.set_seq_form(models.VAE.SEQ_FORM_DEFAULT)
    assert torch.equal(o["ref"], k["ref"])
    assert torch.equal(o["frame_err"][:, 1], k["err_ref"])      # the likelihood row term of the same frame
    tg, pr = k["tgt"].double().cpu().numpy(), k["pred"].double().cpu().numpy()
    close(o["frame_err"][:, 0].cpu().numpy(), np.mean(np.square(tg - pr), axis=1), "err_pred")
    # seq_err: the frame errors summed in double, in frame order
    fe = o["frame_err"].double().cpu().numpy()
    want = np.array([[sum(fe[a:b, j]) for j in range(2)] for a, b in zip(k["off"][:-1], k["off"][1:])])
    got = o["seq_err"].cpu().numpy()
    assert got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=1e-15, atol=0)
    assert got[LENS.index(0)].tolist() == [0.0, 0.0]
    # ref alone, without a target, is the same ref
    assert torch.equal(m.filter_sequences(k["pred"], k["off"], eps=k["eps"])["ref"], k["ref"])


@pytest.mark.parametrize("name", list(SHAPES))
def test_order_independence(name):
    """Another order of the sequences puts other rows into a tile and makes another tile the longest."""
    m, k = model_of(name), case_of(name)
    whole = m.filter_sequences(k["pred"], k["off"], eps=k["eps"], target=k["tgt"], want=("ref", "frame_err"))
    perm = np.random.default_rng(9).permutation(len(LENS))
    idx = np.concatenate([np.arange(k["off"][s], k["off"][s + 1]) for s in perm])
    idx_d = torch.from_numpy(idx).cuda()
    o = m.filter_sequences(k["pred"][idx_d], offsets([LENS[s] for s in perm]), eps=k["eps"][idx_d],
                           target=k["tgt"][idx_d], want=("ref", "frame_err"))
    assert torch.equal(o["ref"], whole["ref"][idx_d])
    assert torch.equal(o["frame_err"], whole["frame_err"][idx_d])


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("at", [1, 2, 7])
@pytest.mark.parametrize("name", list(SHAPES))
def test_chunked_calls_equal_one_call(name, at, form):
    m, k = model_of(name), case_of(name)
    i1, o1, i2, o2 = so.split(k["off"], at)
    d1, d2 = torch.from_numpy(i1).cuda(), torch.from_numpy(i2).cuda()
    m.set_seq_form(form)
    try:
        whole = m.filter_sequences(k["pred"], k["off"], eps=k["eps"], target=k["tgt"], want=("ref", "frame_err", "seq_err"))
        st = m.new_seq_state(len(LENS))
        a = m.filter_sequences(k["pred"][d1], o1, eps=k["eps"][d1], target=k["tgt"][d1], state=st,
                               want=("ref", "frame_err", "seq_err"))
        started = st[1].cpu().numpy().copy()
        b = m.filter_sequences(k["pred"][d2], o2, eps=k["eps"][d2], target=k["tgt"][d2], state=st,
                               want=("ref", "frame_err", "seq_err"))
    finally:
        m.set_seq_form(models.VAE.SEQ_FORM_DEFAULT)
    assert torch.equal(whole["ref"], k["ref"])
    assert started.tolist() == [int(n > 0) for n in LENS]        # an empty sequence stays unstarted
    assert torch.equal(a["ref"], whole["ref"][d1]) and torch.equal(b["ref"], whole["ref"][d2])
    assert torch.equal(a["frame_err"], whole["frame_err"][d1]) and torch.equal(b["frame_err"], whole["frame_err"][d2])
    np.testing.assert_allclose((a["seq_err"] + b["seq_err"]).cpu().numpy(), whole["seq_err"].cpu().numpy(),
                               rtol=1e-12, atol=0)
    # the empty sequence's state was left as new_seq_state made it
    assert not st[0][LENS.index(0)].any()


@pytest.mark.parametrize("form", [0, 1])
def test_integer_model_bit_exact(form):
    k = so.exact_case()
    shape = k["shape"]
    m = models.VAE(shape[0], shape[2], shape[1], shape[3], shape[4], max_batch=64, seed=1)
    m.set_weights(k["P"])
    m.set_seq_form(form)
    o = m.filter_sequences(np.array(k["pred"]), np.array(k["seq_off"]), eps=np.array(k["eps"]))
    np.testing.assert_array_equal(o["ref"].cpu().numpy(), k["ref"])
    m.close()


def test_free_running_vs_float64_oracle():
    name, shape = "in144", SHAPES["in144"]
    m = model_of(name)
    S, T = 20, 64
    rng = np.random.default_rng(21)
    off = np.arange(S + 1, dtype=np.int64) * T
    pred = rng.standard_normal((S * T, 48)).astype(np.float32)
    eps = rng.standard_normal((S * T, 24)).astype(np.float32)
    tgt = rng.standard_normal((S * T, 48)).astype(np.float32)
    want = so.filter(rand_params(shape, 3), shape, pred, off, eps, target=tgt)
    o = m.filter_sequences(pred, off, eps=eps, target=tgt, want=("ref", "frame_err", "seq_err"))
    ref = o["ref"].cpu().numpy()
    print("free-running |d| max %.3g, frame_err |d| max %.3g" % (
        np.abs(ref - want["ref"]).max(), np.abs(o["frame_err"].cpu().numpy() - want["frame_err"]).max()))
    close(ref, want["ref"], "ref")
    close(o["frame_err"].cpu().numpy(), want["frame_err"], "frame_err")
    np.testing.assert_allclose(o["seq_err"].cpu().numpy(), want["seq_err"], rtol=1e-5, atol=0)


@pytest.mark.parametrize("name", list(SHAPES))
def test_internal_eps_equals_the_eps_kernel(name):
    m, k = model_of(name), case_of(name)
    c, r = 11, 1000
    a = m.filter_sequences(k["pred"], k["off"], eps=None, ctr=c, eps_row0=r)["ref"]
    b = m.filter_sequences(k["pred"], k["off"], eps=m.eps_device(k["N"], ctr=c, row0=r))["ref"]
    assert torch.equal(a, b)
    assert not torch.equal(a, m.filter_sequences(k["pred"], k["off"], eps=None, ctr=c + 1, eps_row0=r)["ref"])


@pytest.mark.parametrize("form", [0, 1])
def test_only_the_frames_are_written(form):
    """ref and frame_err filled with NaN beforehand: rows [0, N) are overwritten, a guard row past N
    keeps its NaN."""
    m, k = model_of("in144"), case_of("in144")
    N, S = k["N"], len(LENS)
    ref = torch.full((N + 1, 48), float("nan"), device="cuda")
    fe = torch.full((N + 1, 2), float("nan"), device="cuda")
    se = torch.full((S + 1, 2), float("nan"), device="cuda", dtype=torch.float64)
    off = torch.from_numpy(k["off"]).cuda()
    m.set_seq_form(form)
    try:
        _p3d.check(_p3d.lib().p3d_vae_seq_filter(m._h, ptr(k["pred"]), ptr(off), S, N, ptr(k["eps"]), 0, 0, ptr(k["tgt"]),
                                                 None, None, ptr(ref), ptr(fe), ptr(se), m.stream()), "p3d_vae_seq_filter")
    finally:
        m.set_seq_form(models.VAE.SEQ_FORM_DEFAULT)
    torch.cuda.synchronize()
    assert torch.equal(ref[:N], k["ref"]) and torch.isnan(ref[N]).all()
    assert not torch.isnan(fe[:N]).any() and torch.isnan(fe[N]).all()
    assert not torch.isnan(se[:S]).any() and torch.isnan(se[S]).all()


def test_argument_errors():
    m, k = model_of("in144"), case_of("in144")
    with pytest.raises(ValueError):
        m.filter_sequences(k["pred"][:, :40], k["off"], eps=k["eps"])                      # a wrong width
    with pytest.raises(ValueError):
        m.filter_sequences(k["pred"], k["off"], eps=k["eps"][:, :16])
    with pytest.raises(ValueError):
        m.filter_sequences(k["pred"][:-1], k["off"], eps=k["eps"][:-1])                    # offsets do not end at N
    with pytest.raises(ValueError):
        m.filter_sequences(k["pred"], k["off"][::-1].copy(), eps=k["eps"])
    with pytest.raises(ValueError):
        m.filter_sequences(k["pred"], k["off"], eps=k["eps"], want=("ref", "frame_err"))   # no target
    with pytest.raises(ValueError):
        m.filter_sequences(k["pred"], k["off"], eps=k["eps"], state=(torch.zeros(3, 96, device="cuda"),
                                                                     torch.zeros(3, dtype=torch.int32, device="cuda")))
    odd = models.VAE(80, 24, (40, 32), (32, 40), 48, max_batch=64, seed=1)                 # in is no multiple of out
    with pytest.raises(ValueError):
        odd.filter_sequences(k["pred"], k["off"])
    with pytest.raises(ValueError):
        odd.new_seq_state(4)
    # the library refuses the same on its own
    off = torch.from_numpy(k["off"]).cuda()
    out = torch.empty_like(k["pred"])
    lib = _p3d.lib()
    assert lib.p3d_vae_seq_filter(odd._h, ptr(k["pred"]), ptr(off), 33, k["N"], None, 0, 0, None, None, None, ptr(out),
                                  None, None, None) == _p3d.P3D_ERR_ARG
    fe = torch.empty((k["N"], 2), device="cuda")
    assert lib.p3d_vae_seq_filter(m._h, ptr(k["pred"]), ptr(off), 33, k["N"], None, 0, 0, None, None, None, ptr(out),
                                  ptr(fe), None, None) == _p3d.P3D_ERR_ARG
    assert lib.p3d_vae_seq_filter(m._h, ptr(k["pred"]), ptr(off), 33, (1 << 20) + 1, None, 0, 0, None, None, None,
                                  ptr(out), None, None, None) == _p3d.P3D_ERR_ARG
    assert lib.p3d_vae_seq_set_form(m._h, 2) == _p3d.P3D_ERR_ARG
    odd.close()


def test_graph_replays():
    m, k = model_of("in144"), case_of("in144")
    off = torch.from_numpy(k["off"]).cuda()
    pred = k["pred"].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.filter_sequences(pred, off, eps=k["eps"], target=k["tgt"], want=("ref", "frame_err"))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        o = m.filter_sequences(pred, off, eps=k["eps"], target=k["tgt"], want=("ref", "frame_err"))
    eager = m.filter_sequences(k["pred"], k["off"], eps=k["eps"], target=k["tgt"], want=("ref", "frame_err"))
    for _ in range(2):
        o["ref"].fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o["ref"], eager["ref"]) and torch.equal(o["frame_err"], eager["frame_err"])
    # the graph reads its inputs anew at every replay
    pred.mul_(0.5)
    g.replay()
    torch.cuda.synchronize()
    half = m.filter_sequences(pred, off, eps=k["eps"])["ref"]
    assert torch.equal(o["ref"], half) and not torch.equal(half, eager["ref"])


def test_driver_trains_and_evaluates_against_the_oracle(tmp_path):
    """3d_pose_vae_filter_kin on synthetic H3.6M archives: train() runs two short epochs on noised
    windows and the test ELBO falls; evaluate() -- the lifter once over all test frames, then one
    filter_sequences call -- returns per-key and overall errors equal to the float64 oracle's
    recurrence over the same lifter outputs and eps rows."""
    import importlib.util
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "golden"))
    from synth_cameras import write_h36m_archives
    tree, camsp = str(tmp_path / "h36m.npz"), str(tmp_path / "cameras.npz")
    write_h36m_archives(tree, camsp, np.random.default_rng(31), ["Walking", "Directions"], frames=400, sh=False)
    np.random.seed(5)
    spec = importlib.util.spec_from_file_location(
        "pose_vae_filter_kin", os.path.join(os.path.dirname(here), "3d-pose-baseline_amd", "3d_pose_vae_filter_kin.py"))
    kin = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kin)
    # the reference's own settings (src/train.yml): lr 1e-4, factors 100 / 0.02 / 1, as in
    # tests/test_gpu_vae.py's train() test and for its reason: the test subjects have other cameras, so
    # what carries over to the test set is the early, slow descent of the likelihood term (at 1e-3 the
    # filter fits the training subjects within two epochs and the test ELBO turns: 143.1 -> 149.7)
    cfg = tmp_path / "train.yml"
    cfg.write_text("train:\n  step_log: 2000\n  learning_rate: 0.0001\n  likelihood_factor: 100.0\n"
                   "  kcs_factor: 0.02\n  dkl_factor: 1.0\n")
    argv = ["--camera_frame", "--action", "Walking", "--data_dir", tree, "--cameras_path", camsp,
            "--linear_size", "128", "--num_layers", "1", "--residual", "--batch_norm", "--cfg_file", str(cfg),
            "--train_dir", str(tmp_path / "vae"), "--epochs", "2", "--seed", "3"]
    model, hist = kin.train(argv, read_from_config=True)
    assert kin.ENV.FLAGS.learning_rate == 1e-4 and list(kin.ENV.FLAGS.noise_3d) == [1, 1]
    assert model.input_size == 144 and model.get_step()[0] > 0
    assert len(hist["loss_test"]) == 2 and np.isfinite(hist["loss_test"]).all()
    print("test ELBO per epoch", hist["loss_test"], "prediction error", hist["pred_error"])
    assert hist["loss_test"][1].sum() < hist["loss_test"][0].sum()
    saved = kin.weights_path() + ".npz"
    weights = dict(zip([n for n, _, _ in model.param_table], model.get_weights()))
    model.close()
    res = kin.evaluate(argv + ["--evaluate", "--vae_weights", saved], read_from_config=True)
    vae, off = res["vae"], res["seq_off"]
    N = int(off[-1])
    assert len(res["keys"]) == len(res["per_key"]) == len(off) - 1 > 1 and N == res["pred"].shape[0]
    for n, w in zip([n for n, _, _ in vae.param_table], vae.get_weights()):
        np.testing.assert_array_equal(w, weights[n])
    eps = vae.eps_device(N, ctr=res["eps_ctr"], row0=0).cpu().numpy()
    want = so.filter(weights, SHAPES["in144"], res["pred"].cpu().numpy(), off, eps, target=res["target"].cpu().numpy())
    close(res["ref"].cpu().numpy(), want["ref"], "ref")
    lens = np.diff(off)
    for i, key in enumerate(res["keys"]):
        np.testing.assert_allclose(res["per_key"][key], want["seq_err"][i] / lens[i], rtol=1e-5, atol=0)
    np.testing.assert_allclose(res["overall"], want["seq_err"].sum(axis=0) / N, rtol=1e-5, atol=0)
    e1 = want["frame_err"][:, 0]
    np.testing.assert_allclose(res["noise"], (e1.mean(), e1.std(), e1.min(), e1.max()), rtol=1e-5, atol=0)
    vae.close()
    res["pose3d"].close()
