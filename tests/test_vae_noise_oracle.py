"""CPU tests of the device noise stream's oracle (tests/vae_noise_oracle.py), of the host add_noise
against the same statistics, of the host half of load_3d_data / Dataset, and of p3d_vae_add_noise's
argument errors (which answer without a GPU)."""
import ctypes
import math
import os
import types

import numpy as np
import pytest

import vae_noise_oracle as no
import vae_oracle as vo
from top_vae_3d_pose import data_handler

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3d-pose-baseline_amd", "libp3d.so")
Z_BOUND = 5.0      # standard errors, every statistic


def test_threshold_literal_is_phi_of_a_half():
    phi = 0.5 * (1 + math.erf(0.5 / math.sqrt(2)))
    assert 0xB103AF11 == math.floor(phi * 2 ** 32) == no.THRESHOLD
    assert abs(phi - 0.6914624612740131) < 1e-15
    assert (no.NOISE, no.NOISE_OFFSET) == (data_handler.NOISE, data_handler.NOISE_OFFSET)
    assert len({no.NOISE_SITE, no.NOISE_ROW_SITE, vo.EPS_SITE}) == 3 and min(no.NOISE_SITE, no.NOISE_ROW_SITE) >= 64
    assert data_handler.joint_scale([1, 1]) == np.float32(1.22108747) and data_handler.joint_scale([7, 0.5]).dtype == np.float32


def test_normals4_is_the_eps_streams_box_muller():
    rows = np.arange(5, 69, dtype=np.uint32)[:, None]
    e = no.normals4(rows, np.arange(6, dtype=np.uint32)[None, :], vo.EPS_SITE, (9 << 32) | 77, 3).reshape(64, 24)
    np.testing.assert_array_equal(e.view(np.uint32), vo.eps_stream((9 << 32) | 77, 3, 5, 64, 24).view(np.uint32))


def test_stream_definition_on_a_few_rows():
    """noise_stream against a scalar, row-by-row restatement of the definition in include/p3d.h."""
    from oracle import ref_mlp
    rng = np.random.default_rng(2)
    seed, ctr, row0, width = (3 << 32) | 11, (1 << 32) | 6, (1 << 32) - 3, 24     # (row and ctr wrap at 32 bits)
    x = rng.standard_normal((9, width)).astype(np.float32)
    out, mask, jid, e, j = no.noise_stream(x, seed, ctr, row0=row0, noise_3d=[1, 0.5])
    scale = np.float32(no.NOISE + 0.5)
    f32 = np.float32
    for r in range(9):
        g = np.uint32((row0 + r) & 0xFFFFFFFF)
        A = [int(np.asarray(w)) for w in ref_mlp.philox4x32_10(g, np.uint32(0), np.uint32(no.NOISE_ROW_SITE),
                                                               np.uint32(ctr & 0xFFFFFFFF), np.uint32(seed & 0xFFFFFFFF),
                                                               np.uint32(seed >> 32))]
        assert bool(mask[r]) == (A[0] >= 0xB103AF11)
        jc = (A[1] * width) >> 32
        assert jid[r] == jc - jc % 3 and 0 <= jid[r] <= width - 3
        if not mask[r]:
            np.testing.assert_array_equal(out[r].view(np.uint32), x[r].view(np.uint32))
            continue
        v = [f32(x[r, c] + f32(f32(e[r, c] * f32(no.NOISE)) + f32(no.NOISE_OFFSET))) for c in range(width)]
        for k in range(3):
            v[jid[r] + k] = f32(v[jid[r] + k] + f32(j[r, k] * scale))
        np.testing.assert_array_equal(np.array(v, f32).view(np.uint32), out[r].view(np.uint32))
    assert mask.any() and not mask.all()


@pytest.mark.parametrize("width", [48, 144])
def test_oracle_statistics(width):
    n = 1 << 16
    x = np.random.default_rng(width).standard_normal((n, width)).astype(np.float32)
    out, mask, jid, _, _ = no.noise_stream(x, seed=5, ctr=2, noise_3d=[1, 1])
    z, m = no.statistics(x, out, [1, 1], jid=jid)
    print("oracle, width %d: %d noised rows, z scores %s" % (width, m, z))
    assert m == int(mask.sum())
    assert all(abs(v) <= Z_BOUND for v in z.values()), z
    z2, _ = no.statistics(x, out, [1, 1])          # the joint read off the output, as for the host add_noise
    assert abs(z2["joint"]) <= Z_BOUND, z2


@pytest.mark.parametrize("width", [48, 144])
def test_host_add_noise_meets_the_same_statistics(width):
    n = 1 << 16
    x = np.random.default_rng(width + 1).standard_normal((n, width)).astype(np.float32)
    np.random.seed(0)
    out = data_handler.add_noise(x, [1, 1])
    z, m = no.statistics(x, out, [1, 1])
    print("host add_noise, width %d: %d noised rows, z scores %s" % (width, m, z))
    assert all(abs(v) <= Z_BOUND for v in z.values()), z


def _synthetic_dict(rng):
    tr = {(1, "Walking", "a.h5"): rng.standard_normal((37, 48)), (5, "Walking", "b.h5"): rng.standard_normal((20, 48)),
          (1, "Eating", "c.h5"): rng.standard_normal((11, 48))}
    te = {(9, "Walking", "a.h5"): rng.standard_normal((23, 48)), (11, "Eating", "d.h5"): rng.standard_normal((12, 48))}
    return dict(train_set_3d=tr, test_set_3d=te, data_mean_3d=np.zeros(96), data_std_3d=np.ones(96),
                dim_to_ignore_3d=np.arange(48, 96), dim_to_use_3d=np.arange(48))


def test_split_3d_data_sizes_and_key_order():
    d = _synthetic_dict(np.random.default_rng(3))
    joined = data_handler.join_data(d["train_set_3d"], d["test_set_3d"], list(d["train_set_3d"]), list(d["test_set_3d"]))
    assert joined.dtype == np.float32 and joined.shape == (103, 48)
    want = np.concatenate([d["train_set_3d"][k] for k in d["train_set_3d"]] + [d["test_set_3d"][k] for k in d["test_set_3d"]])
    np.testing.assert_array_equal(joined, want.astype(np.float32))       # train keys, then test keys, in dict order
    np.random.seed(4)
    train, test, meta = data_handler.split_3d_data(d)
    np.random.seed(4)
    idx = np.random.choice(103, 103, replace=False)
    assert train.shape == (82, 48) and test.shape == (21, 48)            # int(103 * 0.8) = 82
    np.testing.assert_array_equal(train, joined[idx[:82]])
    np.testing.assert_array_equal(test, joined[idx[82:]])
    assert meta._fields == ("mean", "std", "dim_ignored", "dim_used")
    assert meta.mean is d["data_mean_3d"] and meta.dim_used is d["dim_to_use_3d"]


def test_dataset_len_is_the_floor():
    ln = data_handler.Dataset.__len__
    assert ln(types.SimpleNamespace(shape=(130, 48), batch_size=64)) == 2
    assert ln(types.SimpleNamespace(shape=(128, 48), batch_size=64)) == 2
    assert ln(types.SimpleNamespace(shape=(63, 48), batch_size=64)) == 0


def test_dataset_needs_a_gpu_and_says_so():
    import torch
    with pytest.raises(ValueError):      # (a host array is refused, GPU or not: nothing is moved silently)
        data_handler.add_noise_device(np.zeros((8, 48), np.float32), seed=0, ctr=0)
    with pytest.raises(ValueError):
        data_handler.add_noise_device(torch.zeros((8, 48)), seed=0, ctr=0)
    if not torch.cuda.is_available():    # (with one, tests/test_gpu_vae_noise.py covers Dataset)
        import _p3d
        with pytest.raises(_p3d.P3DError):
            data_handler.Dataset(np.zeros((8, 48), np.float32))


def test_add_noise_argument_errors_without_a_gpu():
    if not os.path.exists(LIB):
        pytest.skip("libp3d.so not built")
    import _p3d
    lib, E = _p3d.lib(), _p3d.P3D_ERR_ARG
    buf = (ctypes.c_float * 4096)()
    a = ctypes.addressof(buf)
    a += (-a) % 16
    src, out, st = ctypes.c_void_p(a), ctypes.c_void_p(a + 8192), ctypes.c_void_p(a + 4096)

    def call(src=src, rows=8, d=48, starts=None, width=48, B=8, out=out):
        rc = lib.p3d_vae_add_noise(src, rows, d, starts, width, B, 1, 0, 0, 0.2, 0.001, 1.2, out, None)
        if rc == E:
            assert lib.p3d_last_error().decode().startswith("p3d_vae_add_noise: ")
        return rc

    assert call(width=10, d=10) == E and call(width=10, d=2) == E                # below 12, not a multiple of 12
    assert call(width=252, d=252) == E and call(width=252, d=84) == E            # above 240
    assert call(width=20, d=20) == E                                             # a multiple of 4, not of 12
    assert call(width=144, d=96, starts=st) == E                                 # not a multiple of d
    assert call(width=48, d=24) == E                                             # the plain form needs width == d
    assert call(width=12, d=6, starts=st) == E and call(width=36, d=18, starts=st) == E   # d no multiple of 4
    assert call(B=0) == E and call(B=(1 << 20) + 1, rows=(1 << 20) + 1) == E
    assert call(src=None) == E and call(out=None) == E
    assert call(src=ctypes.c_void_p(a + 4)) == E and call(out=ctypes.c_void_p(a + 8192 + 8)) == E
    assert call(starts=ctypes.c_void_p(a + 4096 + 4), width=144, rows=40) == E   # starts: 8 bytes
    assert call(rows=7) == E                                                     # rows < B without starts
    assert call(starts=st, width=144, rows=40, out=src) == E                     # the window form in place
    assert call(starts=st, width=144, rows=40, out=ctypes.c_void_p(a + 48 * 4 * 39)) == E   # ... or overlapping
    assert call(starts=st, width=144, rows=2) == E                               # fewer rows than a window
    assert call(out=ctypes.c_void_p(a + 16)) == E                                # plain: overlapping but not src
    assert lib.p3d_vae_add_noise_thr(src, 8, 48, None, 48, 8, 1, 0, 0, 0.2, 0.001, 1.2, (1 << 32) + 1, out, None) == E
