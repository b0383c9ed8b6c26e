"""CPU tests of the decoder's oracle (tests/vae_dec_oracle.py) and of the host side of
p3d_vae_decode: the oracle against the forward oracles, the prior stream's site, the decoder
kernels' LDS and the argument errors that answer without a GPU."""
import ctypes

import numpy as np
import pytest

import _p3d
import vae_bones_oracle as vb
import vae_dec_oracle as vd
import vae_noise_oracle as no
import vae_oracle as vo

SHAPES = {"default": vo.DEFAULT_SHAPE, "edge": (48, (8,), 8, (24,), 48)}
BONES_SHAPES = {"default": vb.DEFAULT_SHAPE, "narrow": (64, (40, 32), 24, (32, 40))}


def _ints(v):
    return (ctypes.c_int32 * len(v))(*v)


def _biased(P, seed):
    rng = np.random.default_rng(seed)
    for k in P:
        if k.endswith("/bias"):
            P[k] = (0.1 * rng.standard_normal(P[k].shape)).astype(np.float32)
    return P


@pytest.mark.parametrize("name", list(SHAPES))
def test_decode_equals_the_forward_oracles_decoder(name):
    shape = SHAPES[name]
    P = _biased(vo.init_params(shape, 3), 4)
    rng = np.random.default_rng(11)
    x = rng.standard_normal((37, shape[0])).astype(np.float32)
    eps = rng.standard_normal((37, shape[2])).astype(np.float32)
    c = vo.forward(P, shape, x, eps)
    y = vd.decode(P, shape, c["z"])
    assert y.dtype == np.float64 and y.shape == (37, shape[4])
    np.testing.assert_array_equal(y, c["y"])
    c32 = vo.forward(P, shape, x, eps, dt=np.float32)
    np.testing.assert_array_equal(vd.decode(P, shape, c32["z"], dt=np.float32), c32["y"])


@pytest.mark.parametrize("name", list(BONES_SHAPES))
def test_decode_bones_equals_the_bones_oracles_decoder(name):
    shape = BONES_SHAPES[name]
    P = _biased(vb.init_params(shape, 3), 4)
    rng = np.random.default_rng(12)
    x = rng.standard_normal((21, shape[0])).astype(np.float32)
    eps = rng.standard_normal((21, shape[2])).astype(np.float32)
    c = vb.forward(P, shape, x, eps)
    y = vd.decode_bones(P, shape, c["z"])
    assert y.shape == (21, 64)
    np.testing.assert_array_equal(y, c["y"])


def test_prior_site_is_a_stream_of_its_own():
    assert vd.PRIOR_SITE == 0x505249
    assert vd.PRIOR_SITE not in (vo.EPS_SITE, no.NOISE_SITE, no.NOISE_ROW_SITE) and vd.PRIOR_SITE >= 64
    seed, ctr, n, lat = 5, 3, 512, 24
    prior = vd.prior_stream(seed, ctr, 0, n, lat)
    eps = vo.eps_stream(seed, ctr, 0, n, lat)
    rows = np.arange(n, dtype=np.uint32)[:, None]
    c4 = np.arange(lat // 4, dtype=np.uint32)[None, :]
    np.testing.assert_array_equal(no.normals4(rows, c4, vo.EPS_SITE, seed, ctr).reshape(n, lat), eps)
    assert not (prior == eps).any(axis=1).all()
    assert (prior != eps).mean() > 0.99
    # keyed by the global row: rows 100 .. of one stream are the stream begun at row0 = 100
    np.testing.assert_array_equal(prior[100:164], vd.prior_stream(seed, ctr, 100, 64, lat))
    assert (vd.prior_stream(seed, ctr + 1, 0, n, lat) != prior).mean() > 0.99


def _dec_lds(shape, bones=0):
    dec = shape[3]
    out = 64 if bones else shape[4]
    return int(_p3d.lib().p3d_vae_dec_lds_bytes(shape[2], len(dec), _ints(dec), out, bones))


def test_dec_lds_bytes():
    lib = _p3d.lib()
    i, enc, lat, dec, out = vo.DEFAULT_SHAPE
    full = int(lib.p3d_vae_lds_bytes(i, len(enc), _ints(enc), lat, len(dec), _ints(dec), out))
    got = _dec_lds(vo.DEFAULT_SHAPE)
    assert 0 < got <= 163840 and got < full, (got, full)
    # the layout, restated: the decoder's packed layers (rows staggered by 4 floats, N padded to 16,
    # the bias behind each) and four areas of the z tile and the layers' outputs (row stride Np + 2)
    c16 = lambda n: (n + 15) // 16 * 16
    widths = list(dec) + [out]
    pk = sum(K * (c16(N) + 4) + c16(N) for K, N in zip([lat] + widths[:-1], widths))
    act = 16 * (c16(lat) + 2) + sum(16 * (c16(N) + 2) for N in widths)
    assert got == 4 * ((pk + 3) // 4 * 4 + 4 * ((act + 3) // 4 * 4))
    b = _dec_lds(vb.DEFAULT_SHAPE, bones=1)
    bfull = int(lib.p3d_vae_bones_lds_bytes(1376, 2, _ints([40, 32]), 24, 2, _ints([32, 40])))
    assert 0 < b < bfull and b > got          # (the bones decoder adds mag1 and a 64-wide output)
    # refused shapes answer 0: a width that is no multiple of 8, a latent past 64, five layers, bones not 0 / 1
    assert _dec_lds((48, (40,), 24, (32, 41), 48)) == 0
    assert _dec_lds((48, (40,), 72, (32, 40), 48)) == 0
    assert _dec_lds((48, (40,), 24, (32, 40, 48, 56, 64), 48)) == 0
    assert int(lib.p3d_vae_dec_lds_bytes(24, 2, _ints([32, 40]), 48, 2)) == 0
    assert int(lib.p3d_vae_dec_lds_bytes(24, 2, None, 48, 0)) == 0


def test_decode_argument_errors_answer_without_a_gpu():
    lib = _p3d.lib()
    y = ctypes.c_void_p(64)             # never dereferenced: every call below is refused before the launch
    ctr_dev = 0xFFFFFFFFFFFFFFFF        # P3D_CTR_GLOBAL_STEP
    cases = [
        ((None, None, 16, 0, 0, y, None, None), "null handle"),
        ((None, None, 16, 0, 0, None, None, None), "y is null"),
        ((None, None, 0, 0, 0, y, None, None), "B must be in 1 .. 2^20"),
        ((None, None, (1 << 20) + 1, 0, 0, y, None, None), "B must be in 1 .. 2^20"),
        ((None, y, 16, 0, 0, y, y, None), "not both"),
        ((None, None, 16, 0, -1, y, None, None), "row0 must be >= 0"),
        ((None, None, 16, ctr_dev, 0, y, None, None), "P3D_CTR_GLOBAL_STEP"),
    ]
    for args, text in cases:
        assert lib.p3d_vae_decode(*args) == _p3d.P3D_ERR_ARG, text
        msg = lib.p3d_last_error().decode()
        assert msg.startswith("p3d_vae_decode: ") and text in msg, msg
    with pytest.raises(ValueError, match="p3d_vae_decode: "):
        _p3d.check(lib.p3d_vae_decode(None, None, 16, 0, 0, y, None, None), "p3d_vae_decode")
    assert lib.p3d_vae_dec_set_grid(None, 1) == _p3d.P3D_ERR_ARG
