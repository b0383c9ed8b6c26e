"""CPU tests of the bones filter's oracle (tests/vae_bones_oracle.py) and of the host side of the
bones entry points: the oracle against an independent torch-autograd statement of the graph, its
conversions against the reference's own (tests/golden/bones_goldens.npz) bit for bit, the yaml
walk against the built-in table, the exactness proof of the integer cases
(tests/vae_bones_exact.py), argument validation without a GPU, the flags."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _p3d
import vae_bones_exact as vx
import vae_bones_oracle as vb

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1376, (40, 32), 24, (32, 40)), (64, (40, 32), 24, (32, 40)), (264, (8,), 8, (8,))]
FACTORS = [(10.0, 100.0, 1.0, 100.0), (1.0, 1.0, 1.0, 1.0), (1.0, 0.0, 0.0, 0.0), (0.0, 0.5, 3.0, 0.0),
           (0.0, 0.0, 0.0, 2.0)]                                                   # first: train.yml's


def _rand(shape, seed, B=5):
    rng = np.random.default_rng(seed)
    P = vb.init_params(shape, seed)
    for k in P:
        if k.endswith("/bias"):
            P[k] = (0.1 * rng.standard_normal(P[k].shape)).astype(np.float32)
    return (P, rng.standard_normal((B, shape[0])), rng.standard_normal((B, shape[2])),
            rng.standard_normal((B, 64)))


def _torch_graph(P, shape, x, eps, t, factors):
    """models.py:544-573 and losses.py:113-156 written with torch ops and autograd (float64)."""
    _, enc, lat, dec = shape
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
    out1 = torch.relu(d @ p["mag1/kernel"] + p["mag1/bias"])
    pred_mag = out1 @ p["mag2/kernel"] + p["mag2/bias"]
    pred_cos = out1 @ p["cos2/kernel"] + p["cos2/bias"]          # cos2 reads mag1's output (models.py:565-566)
    tt = torch.tensor(t)
    mags, dir_cos = tt[:, :16], tt[:, 16:]
    dkl = 0.5 * torch.sum(torch.exp(lv) + mean ** 2 - 1.0 - lv, dim=-1)
    l1 = torch.mean((mags - pred_mag) ** 2, dim=-1)
    l2 = 3.0 * torch.mean((dir_cos - pred_cos) ** 2, dim=-1)
    ang_real = dir_cos.reshape(len(x), -1, 3).permute(0, 2, 1)
    ang_pred = pred_cos.reshape(len(x), -1, 3).permute(0, 2, 1)
    l3m = (ang_real.transpose(1, 2) @ ang_real - ang_pred.transpose(1, 2) @ ang_pred).abs()
    loss = torch.stack([factors[0] * l1.mean(), factors[1] * l2.mean(), factors[2] * dkl.mean(),
                        factors[3] * l3m.mean()])
    loss.sum().backward()
    g = {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in p.items()}
    return dict(mag=pred_mag.detach().numpy(), cos=pred_cos.detach().numpy(), mean=mean.detach().numpy(),
                log_var=lv.detach().numpy(), z=z.detach().numpy(),
                terms=torch.stack([l1, l2, dkl, l3m.mean(dim=(1, 2))], dim=1).detach().numpy(),
                loss=loss.detach().numpy(), g=g)


@pytest.mark.parametrize("factors", FACTORS)
@pytest.mark.parametrize("shape", SHAPES, ids=("wide1376", "narrow64", "edge"))
def test_oracle_matches_torch_autograd(shape, factors):
    """The bounds of tests/test_vae_oracle.py: 1e-10 on values, 1e-7 on gradients."""
    P, x, eps, t = _rand(shape, 3)
    ref = _torch_graph(P, shape, x, eps, t, factors)
    c = vb.forward(P, shape, x, eps)
    for k in ("mag", "cos", "mean", "log_var", "z"):
        assert np.abs(c[k] - ref[k]).max() < 1e-10, k
    assert np.array_equal(c["y"], np.concatenate([c["mag"], c["cos"]], axis=1))
    terms = vb.row_terms(c, t)
    assert np.abs(terms - ref["terms"]).max() < 1e-10
    assert np.abs(vb.loss4(terms, factors) - ref["loss"]).max() < 1e-10
    g, _ = vb.backward(P, shape, c, t, factors)
    assert sorted(g) == sorted(ref["g"]) == sorted(n for n, _ in vb.param_names(shape))
    assert not any(n.startswith("cos1") for n in g)
    for k in g:
        assert np.abs(g[k] - ref["g"][k]).max() < 1e-7, k


def test_ang_gradient_is_zero_on_identical_cosines():
    """sign(0) = 0: a prediction equal to the target gives a zero dy, not a NaN."""
    shape = SHAPES[1]
    P, x, eps, _ = _rand(shape, 9)
    c = vb.forward(P, shape, x, eps)
    _, dy = vb.backward(P, shape, c, c["y"], (1.0, 1.0, 0.0, 1.0))
    assert not dy.any()


def _same_bits(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=what)
    view = np.uint32 if got.dtype == np.float32 else np.uint64
    ok = np.isnan(ref) | (got.view(view) == ref.view(view))
    assert ok.all(), (what, int((~ok).sum()))


def test_conversions_match_the_reference_bit_for_bit():
    with np.load(os.path.join(HERE, "golden", "bones_goldens.npz")) as z:
        g = {k: z[k] for k in z.files}
    np.testing.assert_array_equal(g["bja"], vb.BJA)
    np.testing.assert_array_equal(g["bjb"], vb.BJB)
    assert np.isnan(g["cos"]).any()
    b = vb.bones_from_joints(g["joints"], np.float64)
    _same_bits(b[:, :16], g["mag"], "mag")
    _same_bits(b[:, 16:], g["cos"], "cos")
    _same_bits(vb.bones_to_joints(np.concatenate([g["mag"], g["cos"]], axis=1)), g["back"], "back")
    _same_bits(vb.bones_to_joints(np.concatenate([g["free_mag"], g["free_cos"]], axis=1)), g["free_back"], "free_back")
    # the float32 form is the same arithmetic one precision down: within 4 float32 ulps of the precise one
    b32 = vb.bones_from_joints(g["joints"], np.float32)
    np.testing.assert_array_equal(np.isnan(b32), np.isnan(b))
    fin = ~np.isnan(b)
    assert (np.abs(b32[fin] - b[fin]) <= 4 * np.spacing(np.abs(b[fin]))).all()
    assert (b32 != b)[fin].any()


def test_yaml_walk_gives_the_builtin_table():
    from top_vae_3d_pose import bones
    mapping = bones.get_bones_mapping(os.path.join(HERE, "golden", "bones_mapping.yml"))
    bja, bjb = bones.get_bones_joints(mapping)
    np.testing.assert_array_equal(bja, bones.BJA)
    np.testing.assert_array_equal(bjb, bones.BJB)
    d_bja, d_bjb = bones.get_bones_joints()
    np.testing.assert_array_equal(d_bja, vb.BJA)
    np.testing.assert_array_equal(d_bjb, vb.BJB)
    produced = {0}
    for a, b in zip(bja, bjb):       # a bone's parent joint is produced by an earlier bone
        assert a in produced
        produced.add(int(b))
    assert produced == set(range(17))
    with pytest.raises(ValueError):
        bones._check_table((np.array(bones.BJA)[::-1], np.array(bones.BJB)))


@pytest.mark.parametrize("B", (16, 64, 128))
@pytest.mark.parametrize("shape", SHAPES[:2], ids=("wide1376", "narrow64"))
def test_integer_cases_are_proven_exact(shape, B):
    k = vx.exact_case(B, shape)
    assert k["factors"] == (8.0 * B, 8.0 * B, float(B), 8.0 * B)
    assert max(k["worst"].values()) < vx.LIMIT
    assert np.abs(k["grads"]["cos2/kernel"]).max() > 0 and np.abs(k["grads"]["enc_h_40/kernel"]).max() > 0


def _ints(v):
    return (ctypes.c_int32 * len(v))(*v)


def test_host_side_argument_checks_need_no_gpu():
    lib = _p3d.lib()
    h = ctypes.c_void_p()
    E = _p3d.P3D_ERR_ARG
    assert lib.p3d_vae_create_bones(1376, 2, _ints([40, 32]), 24, 2, _ints([32, 40]), 64, 1, None) == E
    assert lib.p3d_vae_create_bones(1370, 2, _ints([40, 32]), 24, 2, _ints([32, 40]), 64, 1, ctypes.byref(h)) == E
    assert lib.p3d_vae_create_bones(64, 2, _ints([40, 32]), 24, 5, _ints([32, 40, 8, 16, 24]), 64, 1, ctypes.byref(h)) == E
    assert lib.p3d_vae_create_bones(64, 2, _ints([40, 32]), 24, 2, _ints([32, 40]), 0, 1, ctypes.byref(h)) == E
    assert lib.p3d_vae_create_bones(64, 2, _ints([40, 40]), 24, 2, _ints([32, 40]), 64, 1, ctypes.byref(h)) == E
    assert b"unique" in lib.p3d_last_error()
    assert lib.p3d_vae_kind(None) == -1
    buf = ctypes.c_void_p(4096)
    assert lib.p3d_bones_from_joints(None, 4, 1, buf, None) == E
    assert lib.p3d_bones_from_joints(buf, 0, 1, buf, None) == E
    assert lib.p3d_bones_from_joints(buf, (1 << 20) + 1, 1, buf, None) == E
    assert lib.p3d_bones_from_joints(buf, 4, 2, buf, None) == E
    assert lib.p3d_bones_to_joints(buf, 4, None, None) == E
    assert lib.p3d_bones_to_joints(buf, -1, buf, None) == E
    assert lib.p3d_vae_bones_lds_bytes(1376, 2, _ints([40, 32]), 24, 2, _ints([32, 40])) > 0
    assert lib.p3d_vae_bones_lds_bytes(1377, 2, _ints([40, 32]), 24, 2, _ints([32, 40])) == 0


def test_flags_and_names():
    from top_vae_3d_pose import args_def, losses, models
    f = args_def.build_parser().parse_args([])
    assert (f.mag_factor, f.cos_factor, f.ang_factor) == (1.0, 1.0, 1.0) and isinstance(f.bones_mapping_dir, str)
    f = args_def.build_parser().parse_args(["--mag_factor", "10", "--cos_factor", "100", "--ang_factor", "100",
                                            "--bones_mapping_dir", "x.yml"])
    assert (f.mag_factor, f.cos_factor, f.ang_factor, f.bones_mapping_dir) == (10.0, 100.0, 100.0, "x.yml")
    assert callable(losses.loss_bones) and issubclass(models.VAEBones, models.VAE)
    assert models.VAEBones.N_TERMS == 4 and models.VAE.N_TERMS == 3
    names = [n for n, _ in vb.param_names(SHAPES[0])]
    assert names[-6:] == ["mag1/kernel", "mag1/bias", "mag2/kernel", "mag2/bias", "cos2/kernel", "cos2/bias"]
    assert names[:len(names) - 6] == [n for n, _ in __import__("vae_oracle").param_names(SHAPES[0] + (48,))][:-2]
