"""CPU tests of tests/vae_mc_oracle.py, the statement the K-sample kernels (csrc/p3d_vae_mc.h) are
tested against: K = 1 is the plain oracle exactly, the running fold is the two-pass mean and
variance, c_j is the stated constant, and the argument errors of the three C entry points answer
without a GPU."""
import ctypes
import struct

import numpy as np
import pytest

import _p3d
import vae_mc_oracle as mo
import vae_oracle as vo
import vae_seq_oracle as so

SHAPE = vo.DEFAULT_SHAPE
SEQ_SHAPE = (96, (8,), 8, (24,), 48)


def test_c_is_the_float32_of_the_double_quotient():
    for j in range(mo.MAX_K):
        want = struct.unpack("f", struct.pack("f", 1.0 / float(j + 1)))[0]     # round-to-nearest of the double
        assert mo.c(j).dtype == np.float32 and float(mo.c(j)) == want
        assert mo.c(j, np.float64) == 1.0 / (j + 1)
    assert float(mo.c(0)) == 1.0 and float(mo.c(1)) == 0.5 and float(mo.c(2)) == float(np.float32(1.0 / 3.0))
    # what the GPU tests hand to torch as a Python scalar is this value
    assert all(float(np.float32(1.0 / (k + 1))) == float(mo.c(k)) for k in range(mo.MAX_K))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_one_sample_is_the_plain_forward(dt):
    rng = np.random.default_rng(1)
    P = vo.init_params(SHAPE, 2)
    x = rng.standard_normal((9, 48)).astype(np.float32)
    eps = rng.standard_normal((1, 9, 24)).astype(np.float32)
    o, c = mo.forward(P, SHAPE, x, eps, dt), vo.forward(P, SHAPE, x, eps[0], dt)
    for k in ("y", "mean", "log_var"):
        assert o[k].dtype == dt and np.array_equal(o[k], c[k]), k
    assert not o["y_var"].any()


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_one_sample_is_the_plain_recurrence(dt):
    rng = np.random.default_rng(2)
    P = vo.init_params(SEQ_SHAPE, 3)
    lens = [5, 0, 1, 9]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(off[-1])
    pred = rng.standard_normal((N, 48)).astype(np.float32)
    eps = rng.standard_normal((1, N, 8)).astype(np.float32)
    tgt = rng.standard_normal((N, 48)).astype(np.float32)
    a = mo.filter(P, SEQ_SHAPE, pred, off, eps, target=tgt, dt=dt)
    b = so.filter(P, SEQ_SHAPE, pred, off, eps[0], target=tgt, dt=dt)
    for k in ("ref", "frame_err", "seq_err"):
        assert np.array_equal(a[k], b[k]), k
    assert not a["ref_var"].any()
    # chunks with state give one call's rows, mean fed back included
    eps3 = rng.standard_normal((3, N, 8)).astype(np.float32)
    whole = mo.filter(P, SEQ_SHAPE, pred, off, eps3, target=tgt, dt=dt)
    i1, o1, i2, o2 = so.split(off, 2)
    st = so.new_state(SEQ_SHAPE, len(lens), dt)
    c1 = mo.filter(P, SEQ_SHAPE, pred[i1], o1, eps3[:, i1], target=tgt[i1], state=st, dt=dt)
    c2 = mo.filter(P, SEQ_SHAPE, pred[i2], o2, eps3[:, i2], target=tgt[i2], state=st, dt=dt)
    for k in ("ref", "ref_var", "frame_err"):
        assert np.array_equal(c1[k], whole[k][i1]) and np.array_equal(c2[k], whole[k][i2]), k
    assert whole["ref_var"][off[0]:off[1]].min() > 0


@pytest.mark.parametrize("K", [1, 2, 5, 16, 64])
def test_the_fold_is_the_two_pass_mean_and_variance(K):
    rng = np.random.default_rng(K)
    ys = (3.0 + rng.standard_normal((K, 7, 48))).astype(np.float32)
    mean2 = ys.astype(np.float64).mean(axis=0)
    var2 = np.square(ys.astype(np.float64) - mean2).mean(axis=0)
    m64, v64 = mo.fold(ys, np.float64)
    np.testing.assert_allclose(m64, mean2, rtol=1e-14, atol=0)
    np.testing.assert_allclose(v64, var2, rtol=1e-12, atol=1e-300)
    # float32, every operation rounded once: K - 1 steps of a few ulp each on values of size <= 8
    m32, v32 = mo.fold(ys, np.float32)
    assert m32.dtype == np.float32 and v32.dtype == np.float32
    u = float(np.finfo(np.float32).eps)
    assert np.abs(m32 - mean2).max() <= 2 * K * u * 8
    # the running mean is off by <= K u 8, so is every deviation; d_k^2 then moves by <= 2 |d_k| K u 8, their
    # mean by <= 16 K u mean|d| <= 16 K u sqrt(var); the K products and sums add <= 4 K u var of their own
    assert (np.abs(v32 - var2) <= K * u * (16 * np.sqrt(var2) + 4 * var2 + 1e-6)).all()
    if K == 1:
        assert np.array_equal(m32, ys[0]) and not v32.any()


def test_the_variance_bound_covers_a_perturbation_of_the_samples():
    """var_bound(ys, b) holds for samples moved by up to b each: the pattern that pushes every sample
    away from the mean, and random sign patterns."""
    rng = np.random.default_rng(5)
    K = 5
    ys = rng.standard_normal((K, 64, 48))
    b = 2e-5 + 2e-5 * np.abs(ys).max(axis=0)
    bound = mo.var_bound(ys, b)
    var = np.square(ys - ys.mean(axis=0)).mean(axis=0)
    for trial in range(8):
        sg = np.sign(ys - ys.mean(axis=0)) if trial == 0 else rng.choice([-1.0, 1.0], size=ys.shape)
        yp = ys + sg * b
        varp = np.square(yp - yp.mean(axis=0)).mean(axis=0)
        assert (np.abs(varp - var) <= bound).all()


def test_argument_errors_answer_without_a_gpu():
    """What the three calls refuse before they look at the handle: a null output, K out of range,
    the device counter; then the null handle itself.  (A bones filter's refusal needs a filter:
    tests/test_gpu_vae_mc.py.)"""
    lib = _p3d.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    cat = _p3d.P3DVaeCat()
    ARG = _p3d.P3D_ERR_ARG

    def fwd(K=2, ctr=0, y=p):
        return lib.p3d_vae_forward_mc(None, p, 1, K, None, ctr, y, None, None, None, None)

    def fwd_cat(K=2, ctr=0, y=p):
        return lib.p3d_vae_forward_mc_cat(None, ctypes.byref(cat), 1, K, None, ctr, y, None, None, None, None)

    def seq(K=2, ctr=0, y=p):
        return lib.p3d_vae_seq_filter_mc(None, p, p, 1, 1, K, None, ctr, 0, None, None, None, y, None, None, None, None)

    for call, name in ((fwd, b"p3d_vae_forward_mc:"), (fwd_cat, b"p3d_vae_forward_mc_cat:"), (seq, b"p3d_vae_seq_filter_mc:")):
        assert call(y=None) == ARG
        assert name in lib.p3d_last_error() and b"null" in lib.p3d_last_error()
        for K in (0, -1, 65):
            assert call(K=K) == ARG
            assert b"K must be in 1 .. 64" in lib.p3d_last_error()
        assert call(ctr=_p3d.P3D_CTR_GLOBAL_STEP) == ARG
        assert b"P3D_CTR_GLOBAL_STEP" in lib.p3d_last_error()
        assert call() == ARG                                   # everything else in order: the null handle
        assert name in lib.p3d_last_error()
    with pytest.raises(ValueError):
        _p3d.check(fwd(K=65), "p3d_vae_forward_mc")


def test_the_flag_and_the_python_checks():
    from top_vae_3d_pose import args_def
    p = args_def.build_parser()
    assert p.parse_args([]).filter_samples == 1
    assert args_def.filter_samples(p.parse_args([])) is None
    assert args_def.filter_samples(p.parse_args(["--filter_samples", "3"])) == 3
    for bad in ("0", "65", "-2"):
        with pytest.raises(ValueError):
            args_def.filter_samples(p.parse_args(["--filter_samples", bad]))


def test_the_bones_driver_refuses_the_flag():
    """pose_3d_bones.py --filter_samples K > 1 answers before it loads anything."""
    import importlib.util
    import os
    path = os.path.join(_p3d.HERE, "pose_3d_bones.py")
    spec = importlib.util.spec_from_file_location("pose_3d_bones_mc", path)
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    with pytest.raises(NotImplementedError, match="direction cosines do not average"):
        drv.train(["--filter_samples", "2"])
