"""The VAE filter at the shapes p3d_vae_create accepts beyond the suite's (tests/shape_cases.py's
VAE_SHAPES): all three LDS layouts -- the third, with packed weight strides ld = Np instead of Np + 4
in every contraction, had never run --, three and four layers per side, widths up to 256, latent and
out up to 64, shapes a few hundred bytes under the LDS limit, and the wide form over a deeper core.

Bounds are the project's (tests/test_gpu_vae.py): forward values 2e-5 + 2e-5 |ref| against the float64
oracle, loss vectors 1e-5 relative, gradients 1e-3 of each tensor's largest entry, integer models bit
for bit (tests/test_shape_cases_oracle.py proves them exact and sensitive to a dropped k-group), the
training steps 5e-5 on the weights against the oracle's Keras Adam."""

import numpy as np
import pytest
import torch

import _p3d
import shape_cases as sc
import vae_exact as ve
import vae_oracle as vo
from _p3d import ptr
from test_gpu_vae import _same, _state, close, factors_of, rand_params
from test_gpu_vae_wide import _fresh
from top_vae_3d_pose import models

pytestmark = pytest.mark.gpu

NAMES = list(sc.VAE_SHAPES)
BATCHES = (1, 17, 64, 65, 200)
GRAD_BATCHES = (17, 64, 200)
STEP_BATCHES = (64, 200)
SEQ_LENS = (0, 1, 2, 3, 5, 16, 17, 33, 64)
LR = 1e-3

_models, _cases = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _models.values():
        m.close()
    _models.clear()


def model_of(name):
    """One device model per shape, shared by the read-only tests (weights rand_params(shape, 3))."""
    if name not in _models:
        shape = sc.VAE_SHAPES[name]
        m = models.VAE(shape[0], shape[2], shape[1], shape[3], shape[4], max_batch=256, seed=5)
        m.set_weights(rand_params(shape, 3))
        _models[name] = m
    return _models[name]


RELU_MARGIN = 2e-5     # the forward bound at zero: a result within it cannot change a ReLU's side


def _relu_margin(P, shape, c):
    """The smallest |pre-activation| of any ReLU layer in the float64 forward cache c."""
    ins = list(zip(["enc_h_%d" % u for u in shape[1]], c["enc_in"])) + list(zip(["dec_f_%d" % u for u in shape[3]], c["dec_in"]))
    return min(float(np.abs(a @ P[n + "/kernel"].astype(np.float64) + P[n + "/bias"]).min()) for n, a in ins)


def case_of(name, B):
    """Inputs and the float64 oracle's forward / loss / backward at (shape, B), computed once.  The
    gradient is discontinuous where a ReLU's input crosses zero, and a forward that is right to
    2e-5 may put such an input on the other side (one row's whole contribution to a column of dW,
    far above 1e-3 of the tensor at these batches): the inputs are redrawn until the oracle's every
    ReLU input is at least RELU_MARGIN from zero, so that the gradient bound tests arithmetic."""
    if (name, B) not in _cases:
        shape = sc.VAE_SHAPES[name]
        P = rand_params(shape, 3)
        for attempt in range(64):
            rng = np.random.default_rng([100 * B + len(name), attempt])
            x = rng.standard_normal((B, shape[0])).astype(np.float32)
            t = rng.standard_normal((B, shape[4])).astype(np.float32)
            eps = rng.standard_normal((B, shape[2])).astype(np.float32)
            c = vo.forward(P, shape, x, eps)
            if _relu_margin(P, shape, c) >= RELU_MARGIN:
                break
        else:
            raise AssertionError("%s B=%d: no well-conditioned draw" % (name, B))
        terms = vo.row_terms(c, t)
        g, _ = vo.backward(P, shape, c, t, factors_of(shape))
        _cases[(name, B)] = dict(x=x, t=t, eps=eps, c=c, terms=terms, loss=vo.loss3(terms, factors_of(shape)), g=g)
    return _cases[(name, B)]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", NAMES)
def test_forward_vs_oracle(name, B):
    m, k = model_of(name), case_of(name, B)
    o = m.forward_device(k["x"], eps=k["eps"], target=k["t"], want=("y", "mean", "log_var", "z"))
    for key in ("y", "mean", "log_var", "z"):
        close(o[key].cpu().numpy(), k["c"][key], key)
    close(o["row_terms"].cpu().numpy(), k["terms"], "row_terms")
    loss = m.loss_device(k["x"], k["t"], factors_of(sc.VAE_SHAPES[name]), eps=k["eps"]).cpu().numpy()
    np.testing.assert_allclose(loss, k["loss"], rtol=1e-5, atol=0)


@pytest.mark.parametrize("B", GRAD_BATCHES)
@pytest.mark.parametrize("name", NAMES)
def test_gradients_vs_oracle(name, B):
    m, k = model_of(name), case_of(name, B)
    loss = m.compute_gradients(k["x"], k["t"], factors_of(sc.VAE_SHAPES[name]), eps=k["eps"]).cpu().numpy()
    np.testing.assert_allclose(loss, k["loss"], rtol=1e-5, atol=0)
    g = m.grads()
    assert sorted(g) == sorted(k["g"])
    worst = 0.0
    for n, ref in k["g"].items():
        err = float(np.abs(g[n] - ref).max())
        worst = max(worst, err / float(np.abs(ref).max()))
        assert err <= 1e-3 * np.abs(ref).max(), (n, err, float(np.abs(ref).max()))
    print("grad", name, B, "worst err / max %.3g" % worst)


def _segments(shape, x):
    """x [B, in] of a wide shape as two segments whose concatenation it is: the first columns as they
    are, the rest a (table, index) pair -- the rows stored in another order and gathered back."""
    w0 = 40 if shape[0] < 1000 else 80
    B = x.shape[0]
    perm = np.random.default_rng(B).permutation(B)
    table = np.empty((B, shape[0] - w0), np.float32)
    table[perm] = x[:, w0:]                                   # table[perm[r]] = row r
    dev = torch.device("cuda")
    return [torch.from_numpy(np.ascontiguousarray(x[:, :w0])).to(dev),
            (torch.from_numpy(table).to(dev), torch.from_numpy(perm.astype(np.int64)).to(dev))]


@pytest.mark.parametrize("B", sc.VAE_EXACT_BATCHES)
@pytest.mark.parametrize("name", sc.vae_exact_names())
def test_integer_model_bit_exact(name, B):
    """y, mean, z, the KCS row term and every gradient of the integer model equal the oracle bit for
    bit: form 0 and form 1 at B = 16, form 1 at B = 128, the second run of each over NaN-filled
    gradients and workspace; the wide entries through the cat calls on two segments, one of them
    row-indexed through a permutation."""
    shape = sc.VAE_SHAPES[name]
    k = ve.exact_case(B, shape)
    m = models.VAE(shape[0], shape[2], shape[1], shape[3], shape[4], max_batch=B, seed=1)
    m.set_weights(k["P"])
    xs = [np.array(k["x"])] + ([_segments(shape, k["x"])] if shape[0] > 256 else [])
    for x in xs:
        o = m.forward_device(x, eps=k["eps"], target=k["t"], want=("y", "mean", "z"))
        for key in ("y", "mean", "z"):
            np.testing.assert_array_equal(o[key].cpu().numpy(), k[key], err_msg=key)
        np.testing.assert_array_equal(o["row_terms"][:, 1].cpu().numpy(), k["kcs"])
        for form in ((0, 1) if B <= 64 else (1,)):
            m.set_form(form)
            for run in range(2):
                m.compute_gradients(x, k["t"], k["factors"], eps=k["eps"])
                g = m.grads()
                for n, ref in k["grads"].items():
                    np.testing.assert_array_equal(g[n], ref, err_msg="%s form %d run %d" % (n, form, run))
                m.flat("grads").fill_(float("nan"))
                m.flat("workspace").fill_(float("nan"))
    m.close()


@pytest.mark.parametrize("B", STEP_BATCHES)
@pytest.mark.parametrize("name", NAMES)
def test_three_train_steps(name, B):
    """Three train_step calls give the bits of compute_gradients + adam_apply, and each step, from the
    device's own state before it, lands within 5e-5 of the float64 oracle's Keras Adam step."""
    shape = sc.VAE_SHAPES[name]
    P = rand_params(shape, 12)
    f = factors_of(shape)
    one, two = _fresh(shape, P, max_batch=B), _fresh(shape, P, max_batch=B)
    rng = np.random.default_rng(5 + B)
    worst = 0.0
    for step in range(3):
        x = rng.standard_normal((B, shape[0])).astype(np.float32)
        t = rng.standard_normal((B, shape[4])).astype(np.float32)
        eps = rng.standard_normal((B, shape[2])).astype(np.float32)
        w0, m0, v0 = _state(one)
        l1 = one.train_step_device(x, t, f, LR, eps=eps).clone()
        l2 = two.compute_gradients(x, t, f, eps=eps).clone()
        two.adam_apply(LR)
        torch.cuda.synchronize()
        assert torch.equal(l1, l2), step
        w1 = _state(one)[0]
        gref, _ = vo.backward(w0, shape, vo.forward(w0, shape, x, eps), t, f)
        for n in w0:
            wo, _, _ = vo.adam_apply(w0[n].astype(np.float64), m0[n].astype(np.float64), v0[n].astype(np.float64),
                                     gref[n], LR, step + 1)
            err = float(np.abs(w1[n] - wo).max())
            worst = max(worst, err)
            assert err < 5e-5, (step, n, err)
    print("steps", name, B, "worst weight error %.3g" % worst)
    assert one.get_step()[0] == two.get_step()[0] == 3
    _same(_state(two), _state(one), "grad + adam_apply")
    one.close()
    two.close()


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", sc.VAE_SEQ_NAMES)
def test_sequence_filter_equals_the_per_frame_path(name, form):
    """filter_sequences over 9 sequences of 0 to 64 frames: every frame's bits are those of the
    per-frame forward_device recurrence (tests/test_gpu_vae_seq.py's case_of)."""
    shape, m = sc.VAE_SHAPES[name], model_of(name)
    out, lat, L = shape[4], shape[2], shape[0] // shape[4]
    rng = np.random.default_rng(len(name))
    off = _offsets(SEQ_LENS)
    N = int(off[-1])
    pred = torch.from_numpy(rng.standard_normal((N, out)).astype(np.float32)).cuda()
    eps = torch.from_numpy(rng.standard_normal((N, lat)).astype(np.float32)).cuda()
    lens = torch.tensor(SEQ_LENS, device="cuda")
    offd = torch.from_numpy(off[:-1]).cuda()
    buf = pred[offd.clamp(max=N - 1)].repeat(1, L)
    ref = torch.full((N, out), float("nan"), device="cuda")
    for f in range(max(SEQ_LENS)):
        rows = torch.nonzero(lens > f).flatten()
        g = offd[rows] + f
        x = torch.cat([buf[rows, out:], pred[g]], dim=1)
        y = m.forward_device(x, eps=eps[g])["y"]
        x[:, (L - 1) * out:] = y
        buf[rows] = x
        ref[g] = y
    assert not torch.isnan(ref).any()
    m.set_seq_form(form)
    try:
        got = m.filter_sequences(pred, off, eps=eps)["ref"]
    finally:
        m.set_seq_form(models.VAE.SEQ_FORM_DEFAULT)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("name", [n for n in NAMES if n not in sc.VAE_SEQ_NAMES])
def test_sequence_filter_refuses_the_other_shapes(name):
    """A shape the sequence filter does not serve: p3d_vae_seq_filter returns P3D_ERR_ARG and writes nothing."""
    shape, m = sc.VAE_SHAPES[name], model_of(name)
    N = 8
    pred = torch.zeros((N, shape[4]), device="cuda")
    off = torch.tensor([0, 3, N], dtype=torch.int64, device="cuda")
    out = torch.full((N, shape[4]), 7.0, device="cuda")
    rc = _p3d.lib().p3d_vae_seq_filter(m._h, ptr(pred), ptr(off), 2, N, None, 0, 0, None, None, None, ptr(out),
                                       None, None, None)
    assert rc == _p3d.P3D_ERR_ARG and b"p3d_vae_seq_filter" in _p3d.lib().p3d_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_refused_shape_names_its_bytes_and_leaves_the_library_usable():
    shape, nbytes = sc.VAE_REFUSED
    with pytest.raises(ValueError, match=str(nbytes)):
        models.VAE(shape[0], shape[2], shape[1], shape[3], shape[4], max_batch=64, seed=1)
    k = case_of("w136_edge", 17)
    m = models.VAE(48, 8, (136,), (64,), 48, max_batch=64, seed=1)
    m.set_weights(rand_params(sc.VAE_SHAPES["w136_edge"], 3))
    close(m.forward_device(k["x"], eps=k["eps"])["y"].cpu().numpy(), k["c"]["y"], "y")
    m.close()
