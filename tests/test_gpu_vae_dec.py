"""GPU tests of the decoder on its own (csrc/p3d_vae_dec.h; VAE.decode, VAE.sample,
top_vae_3d_pose/samples.py) against the forward launch, tests/vae_dec_oracle.py and the prior
stream's numpy statement.

Bounds: decode(z) equals the y of forward_device for the same z bit for bit (the same layer function
in the same order on the same packed weights); against the float64 oracle the project's forward
bound 2e-5 + 2e-5 |ref| (tests/test_gpu_vae.py close); the prior stream within EPS_ULPS_BOUND of the
numpy statement, as the eps stream.
"""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import _p3d
import nonfinite_cases as nf
import vae_bones_oracle as vb
import vae_dec_oracle as vd
import vae_oracle as vo
from test_gpu_vae import EPS_ULPS_BOUND, close
from top_vae_3d_pose import bones, data_handler, models

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# name -> (shape, bones, max_batch); a wide filter's forward is bounded by max_batch, decode is not
SHAPES = {
    "default": (vo.DEFAULT_SHAPE, False, 1024),
    "in144": ((144, (40, 32), 24, (32, 40), 48), False, 1024),
    "edge": ((48, (8,), 8, (24,), 48), False, 1024),            # latent 8 and dec 24 pad the MFMA tiles
    "out40": ((48, (40, 32), 24, (32, 40), 40), False, 1024),
    "bones64": ((64, (40, 32), 24, (32, 40)), True, 1024),
    "wide1360": ((1360, (40, 32), 24, (32, 40), 48), False, 64),   # the handle carries the P0 offset
}
BATCHES = (1, 16, 17, 64, 65, 200, 1000)
LDS_LIMIT = 163840


def _ints(v):
    return (ctypes.c_int32 * len(v))(*v)


def dec_wgs(name):
    """Workgroups per CU of the decoder's launch as the host picks them: what a CU's LDS holds, four
    at the most."""
    shape, is_bones, _ = SHAPES[name]
    lds = int(_p3d.lib().p3d_vae_dec_lds_bytes(shape[2], len(shape[3]), _ints(shape[3]), 64 if is_bones else shape[4],
                                               int(is_bones)))
    assert 0 < lds <= LDS_LIMIT
    return min(4, LDS_LIMIT // lds)


def big_batch(name):
    """One 64-row round of the whole grid and 17 rows: waves of the first workgroup take a second tile."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return 64 * cus * dec_wgs(name) + 17


def batches_of(name):
    if name == "wide1360":
        return (1, 17, 64)
    return BATCHES + ("big",)


CASES = [(n, B) for n in SHAPES for B in batches_of(n)]


def rand_params(name, seed):
    shape, is_bones, _ = SHAPES[name]
    P = (vb if is_bones else vo).init_params(shape, seed)
    rng = np.random.default_rng(seed + 1)
    for k in P:
        if k.endswith("/bias"):
            P[k] = (0.1 * rng.standard_normal(P[k].shape)).astype(np.float32)
    return P


_models = {}


def model_of(name):
    """One device model per shape, shared by the tests (none of them changes the weights)."""
    if name not in _models:
        shape, is_bones, mb = SHAPES[name]
        if is_bones:
            m = models.VAEBones(shape[0], shape[2], shape[1], shape[3], max_batch=mb, seed=5)
        else:
            m = models.VAE(shape[0], shape[2], shape[1], shape[3], shape[4], max_batch=mb, seed=5)
        m.set_weights(rand_params(name, 3))
        _models[name] = m
    return _models[name]


def decode64(m, z):
    """The decoder's one output tensor (a bones model's decode returns two views of it)."""
    return models.VAE.decode(m, z)


def bits(t):
    return t.contiguous().view(torch.int32)


def ulps_off(got, ref):
    """The worst deviation in ulps of the reference value (tests/test_gpu_vae.py's eps-stream measure)."""
    return float((np.abs(got.astype(np.float64) - ref) / np.spacing(np.maximum(np.abs(ref), np.float32(1e-30)))).max())


def rows_of(name, B):
    return big_batch(name) if B == "big" else B


@pytest.mark.parametrize("name,B", CASES)
def test_decode_is_the_forwards_decoder_bit_for_bit(name, B):
    """y of forward_device and decode of that forward's z, as int32: every row, the NaN row and the
    Inf row of x included; the other rows have the bits of the finite twin's run."""
    m, B = model_of(name), rows_of(name, B)
    shape = SHAPES[name][0]
    bad_rows = [0] if B == 1 else [B // 2, B - 1]
    x, twin, mask = nf.poisoned((B, shape[0]), bad_rows, 7 * B + len(name), kinds=("nan_first", "pos_inf"))
    eps = np.random.default_rng(B).standard_normal((B, shape[2])).astype(np.float32)
    o = m.forward_device(x, eps=eps, want=("y", "z"))
    y = decode64(m, o["z"])
    assert y.shape == o["y"].shape == (B, m.output_size)
    assert torch.equal(bits(y), bits(o["y"]))
    ot = m.forward_device(twin, eps=eps, want=("y", "z"))
    yt = decode64(m, ot["z"])
    assert torch.equal(bits(yt), bits(ot["y"]))
    y, yt = y.cpu().numpy(), yt.cpu().numpy()
    assert np.isfinite(yt).all()
    np.testing.assert_array_equal(y[~mask].view(np.int32), yt[~mask].view(np.int32))
    assert np.isnan(y[bad_rows[0]]).all()                       # a NaN in x: NaN in every column of z and y
    for r in bad_rows[1:]:
        assert not np.isfinite(y[r]).all()                      # an Inf in x never comes out as a finite row


@pytest.mark.parametrize("name,B", CASES)
def test_decode_vs_float64_oracle(name, B):
    m, B = model_of(name), rows_of(name, B)
    shape, is_bones, _ = SHAPES[name]
    z = np.random.default_rng(3 * B + 1).standard_normal((B, shape[2])).astype(np.float32)
    P = rand_params(name, 3)
    ref = vd.decode_bones(P, shape, z) if is_bones else vd.decode(P, shape, z)
    y = decode64(m, z).cpu().numpy()
    print("decode", name, B, "max |d| %.3g" % np.abs(y - ref).max())
    close(y, ref, "decode %s %d" % (name, B))
    # numpy in, the same bits as a device tensor in; a wrong width is refused
    assert torch.equal(decode64(m, torch.from_numpy(z).cuda()), torch.from_numpy(y).cuda())
    with pytest.raises(ValueError):
        decode64(m, z[:, :-1])


@pytest.mark.parametrize("name", list(SHAPES))
def test_sample_is_decode_of_the_drawn_z(name):
    m = model_of(name)
    for n in (77, big_batch(name)):
        o = models.VAE.sample(m, n, ctr=4, want=("y", "z"))
        assert o["z"].shape == (n, m.latent_dim) and o["y"].shape == (n, m.output_size)
        assert torch.equal(bits(o["y"]), bits(decode64(m, o["z"])))
        tail = min(n, 256)                                        # (the last rows: the ragged tile's)
        assert ulps_off(o["z"][n - tail:].cpu().numpy(), vd.prior_stream(m.seed, 4, n - tail, tail, m.latent_dim)) \
            <= EPS_ULPS_BOUND
    y_only = models.VAE.sample(m, 77, ctr=4)
    assert sorted(y_only) == ["y"]
    assert torch.equal(bits(y_only["y"]), bits(models.VAE.sample(m, 77, ctr=4, want=("y", "z"))["y"]))
    # the grid does not show: one workgroup per CU gives the bits of the default
    n = big_batch(name)
    want = models.VAE.sample(m, n, ctr=4)["y"]
    m.set_dec_grid(1)
    try:
        assert torch.equal(bits(models.VAE.sample(m, n, ctr=4)["y"]), bits(want))
    finally:
        m.set_dec_grid(0)


def test_prior_stream_vs_oracle_and_moments():
    m = model_of("default")
    n = 1 << 16
    o = m.sample(n, ctr=3, want=("y", "z"))
    assert torch.equal(bits(o["y"]), bits(m.decode(o["z"])))
    z = o["z"].cpu().numpy()
    ref = vd.prior_stream(m.seed, 3, 0, n, 24)
    worst = ulps_off(z, ref)
    print("prior stream: worst deviation %.2f ulps of the oracle value" % worst)
    assert worst <= EPS_ULPS_BOUND, worst
    cnt = z.size
    assert abs(z.mean()) < 5 / np.sqrt(cnt)
    assert abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / cnt)
    assert len(np.unique(np.ascontiguousarray(z).reshape(-1, 4).view(np.uint64), axis=0)) == cnt // 4
    # never the eps a training step draws at the same (seed, ctr, row)
    eps = m.eps_device(n, ctr=3).cpu().numpy()
    assert (z != eps).mean() > 0.99


def test_prior_stream_is_keyed_by_the_global_row():
    m = model_of("default")
    a = m.sample(164, ctr=7, want=("y", "z"))
    b = m.sample(64, ctr=7, row0=100, want=("y", "z"))
    for k in ("y", "z"):
        assert torch.equal(bits(a[k][100:]), bits(b[k])), k
    c = m.sample(164, ctr=8, want=("y", "z"))
    assert not torch.equal(a["z"], c["z"]) and not torch.equal(a["y"], c["y"])
    assert (a["z"] != c["z"]).float().mean().item() > 0.99
    other = models.VAE(48, 24, [40, 32], [32, 40], 48, max_batch=16, seed=6, init=False)   # (another seed)
    other.set_weights(rand_params("default", 3))
    assert (other.sample(164, ctr=7, want=("z",))["z"] != a["z"]).float().mean().item() > 0.99
    other.close()
    for bad in (dict(n=0), dict(n=4, row0=-1), dict(n=4, ctr=0xFFFFFFFFFFFFFFFF), dict(n=4, want=("x",))):
        with pytest.raises(ValueError):
            m.sample(**bad)


def test_bones_decode_returns_views_and_joints():
    m = model_of("bones64")
    z = np.random.default_rng(9).standard_normal((37, 24)).astype(np.float32)
    mag, cos = m.decode(z)
    assert tuple(mag.shape) == (37, 16) and tuple(cos.shape) == (37, 48)
    assert mag.untyped_storage().data_ptr() == cos.untyped_storage().data_ptr()
    assert cos.data_ptr() == mag.data_ptr() + 16 * 4 and mag.stride() == cos.stride() == (64, 1)
    y = decode64(m, z)
    assert torch.equal(mag, y[:, :16]) and torch.equal(cos, y[:, 16:])
    joints = bones.convert_to_joints(*m.decode(z))
    assert tuple(joints.shape) == (37, 48) and bool(torch.isfinite(joints).all())
    assert torch.equal(joints, bones.convert_to_joints(y))
    s = m.sample(37, ctr=2, want=("y", "z"))
    smag, scos = s["y"]
    assert tuple(smag.shape) == (37, 16) and tuple(scos.shape) == (37, 48)
    dmag, dcos = m.decode(s["z"])
    assert torch.equal(bits(smag), bits(dmag)) and torch.equal(bits(scos), bits(dcos))
    sj = bones.convert_to_joints(smag, scos)
    assert tuple(sj.shape) == (37, 48) and bool(torch.isfinite(sj).all())


def test_decode_is_capturable():
    m = model_of("default")
    rng = np.random.default_rng(13)
    z = torch.from_numpy(rng.standard_normal((200, 24)).astype(np.float32)).cuda()
    z2 = torch.from_numpy(rng.standard_normal((200, 24)).astype(np.float32)).cuda()
    eager, eager2 = m.decode(z), m.decode(z2)
    eager_s = m.sample(200, ctr=5)["y"]
    buf = z.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.decode(buf)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        y = m.decode(buf)
        ys = m.sample(200, ctr=5)["y"]
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(y), bits(eager)) and torch.equal(bits(ys), bits(eager_s))
    buf.copy_(z2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(y), bits(eager2))


def _load(name, fname):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(HERE), "3d-pose-baseline_amd", fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _archives(tmp_path):
    """Synthetic H3.6M archives and the settings of tests/test_gpu_vae_noise.py's driver test, one epoch."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from synth_cameras import write_h36m_archives
    tree, camsp = str(tmp_path / "h36m.npz"), str(tmp_path / "cameras.npz")
    write_h36m_archives(tree, camsp, np.random.default_rng(31), ["Walking", "Directions"], frames=400, sh=False)
    cfg = tmp_path / "train.yml"
    cfg.write_text("train:\n  step_log: 2000\n  learning_rate: 0.0001\n  likelihood_factor: 100.0\n"
                   "  kcs_factor: 0.02\n  dkl_factor: 1.0\n")
    return ["--camera_frame", "--action", "Walking", "--data_dir", tree, "--cameras_path", camsp,
            "--linear_size", "128", "--num_layers", "1", "--residual", "--batch_norm", "--cfg_file", str(cfg),
            "--train_dir", str(tmp_path / "vae"), "--epochs", "1", "--seed", "3"]


def test_vae_filter_driver_writes_sample_sets(tmp_path):
    import data_utils
    import predict_3dpose
    argv = _archives(tmp_path)
    drv = _load("vae_filter_driver_samples", "vae_filter.py")
    assert drv.ENV.setup(argv=argv).samples_dir == ""                 # off by default
    # without the flag: no file, and np.random is drawn from as before -- the split's permutation and
    # one shuffle of each half's indices at the epoch's end
    np.random.seed(5)
    plain, hist0 = drv.train(argv, read_from_config=True)
    state = np.random.get_state()
    f = drv.ENV.FLAGS
    d = predict_3dpose.load_data(drv._base().lifter_flags(f))
    np.random.seed(5)
    train, test, meta = data_handler.split_3d_data(d)
    idx = np.random.choice(len(test), 9, replace=False)               # what a run with the flag draws next
    np.random.seed(5)
    data_handler.split_3d_data(d)
    np.random.shuffle(np.arange(len(train)))
    np.random.shuffle(np.arange(len(test)))
    ours = np.random.get_state()
    assert state[0] == ours[0] and state[2:] == ours[2:]
    np.testing.assert_array_equal(state[1], ours[1])
    plain.close()
    # with the flag: one file per epoch
    sdir = tmp_path / "samples"
    np.random.seed(5)
    model, hist = drv.train(argv + ["--samples_dir", str(sdir)], read_from_config=True)
    assert sorted(os.listdir(sdir)) == ["samples_0001.npz"]
    with np.load(sdir / "samples_0001.npz", allow_pickle=False) as z:
        s = {k: z[k] for k in z.files}
    assert sorted(s) == ["idx", "noised", "pred", "real"]
    np.testing.assert_array_equal(s["idx"], idx)
    assert s["pred"].shape == (9, 96) and np.isfinite(s["pred"]).all()
    ds = model.data_test
    np.testing.assert_array_equal(ds.data.cpu().numpy(), test)
    real = data_utils.unNormalizeData(test[idx], meta.mean, meta.std, meta.dim_ignored)
    noised1 = data_handler.add_noise_device(ds.data, seed=f.seed, ctr=1)      # the test half's draw of epoch 1
    noised = data_utils.unNormalizeData(noised1.cpu().numpy()[idx], meta.mean, meta.std, meta.dim_ignored)
    assert real.shape == (9, 96)
    np.testing.assert_array_equal(s["real"], real)
    np.testing.assert_array_equal(s["noised"], noised)
    assert not np.array_equal(s["pred"], s["noised"])
    # the samples are written behind the epoch's figures: the history is that of the run without the flag
    for k in hist0:
        np.testing.assert_array_equal(np.asarray(hist[k]), np.asarray(hist0[k]), err_msg=k)
    model.close()
    for flag in ("--noised_sample", "--sample"):
        with pytest.raises(NotImplementedError):
            drv.train(argv + [flag, "--samples_dir", str(sdir)], read_from_config=True)
