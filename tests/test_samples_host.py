"""CPU tests of top_vae_3d_pose/samples.py (the numeric half of gen_sample_img, src/vae_filter.py:22-46)
without a model: the row choice, the shapes and the .npz round trip.

data_utils.unNormalizeData runs on the GPU, so these host tests put its arithmetic, restated in
numpy, in its place; tests/test_gpu_vae_dec.py checks gen_samples against the real one."""
import numpy as np
import pytest

import data_utils
from top_vae_3d_pose import samples

D, N = 96, 40


def _unnormalize(xn, mean, std, ignored):
    """data_utils.unNormalizeData (src/data_utils.py:239-262): the used columns scattered into a
    float32 zero matrix, then * std + mean in float64."""
    used = np.setdiff1d(np.arange(mean.shape[0]), np.asarray(ignored, dtype=np.int64))
    full = np.zeros((xn.shape[0], mean.shape[0]), np.float32)
    full[:, used] = xn
    return full * std.reshape(1, -1) + mean.reshape(1, -1)


@pytest.fixture()
def data(monkeypatch):
    monkeypatch.setattr(data_utils, "unNormalizeData", _unnormalize)
    rng = np.random.default_rng(8)
    ignored = np.sort(rng.choice(D, D - 48, replace=False))
    return dict(real=rng.standard_normal((N, 48)).astype(np.float32),
                noised=rng.standard_normal((N, 48)).astype(np.float32),
                mean=rng.standard_normal(D), std=rng.uniform(0.5, 2.0, D), ignored=ignored)


def test_gen_samples_without_a_model(data):
    np.random.seed(21)
    out = samples.gen_samples(None, data["real"], data["noised"], data["mean"], data["std"], data["ignored"])
    np.random.seed(21)
    idx = np.random.choice(N, 9, replace=False)          # the reference's draw, its first use of np.random
    after = np.random.get_state()[1].copy()
    assert sorted(out) == ["idx", "noised", "real"]
    np.testing.assert_array_equal(out["idx"], idx)
    assert out["idx"].shape == (9,) and out["real"].shape == (9, D) and out["noised"].shape == (9, D)
    assert out["real"].dtype == np.float64
    np.testing.assert_array_equal(out["real"], _unnormalize(data["real"][idx], data["mean"], data["std"], data["ignored"]))
    np.testing.assert_array_equal(out["noised"],
                                  _unnormalize(data["noised"][idx], data["mean"], data["std"], data["ignored"]))
    assert (out["real"][:, data["ignored"]] == data["mean"][data["ignored"]]).all()
    # a given idx is taken as it is and draws nothing
    np.random.seed(21)
    np.random.choice(N, 9, replace=False)
    given = samples.gen_samples(None, data["real"], data["noised"], data["mean"], data["std"], data["ignored"],
                                idx=[3, 1, 2])
    np.testing.assert_array_equal(np.random.get_state()[1], after)
    np.testing.assert_array_equal(given["idx"], [3, 1, 2])
    assert given["real"].shape == (3, D)
    with pytest.raises(ValueError):
        samples.gen_samples(None, data["real"], data["noised"], data["mean"], data["std"], data["ignored"], idx=[N])
    with pytest.raises(ValueError):
        samples.gen_samples(None, data["real"], data["noised"][:-1], data["mean"], data["std"], data["ignored"])


def test_npz_round_trip(data, tmp_path):
    path = samples.sample_path(str(tmp_path), 7)
    assert path.endswith("samples_0007.npz")
    out = samples.gen_samples(None, data["real"], data["noised"], data["mean"], data["std"], data["ignored"],
                              idx=np.arange(9), path=path)
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(out)
        for k in out:
            np.testing.assert_array_equal(z[k], out[k])
            assert z[k].dtype == out[k].dtype


def test_module_draws_no_pictures():
    import sys
    src = open(samples.__file__).read()
    assert "matplotlib" not in src.replace("does not depend on a plotting library", "")
    assert "import matplotlib" not in src and "pyplot" not in src
    assert "--samples_dir" in __import__("top_vae_3d_pose.args_def", fromlist=["x"]).build_parser().format_help()
    assert sys.modules["top_vae_3d_pose.samples"].NSAMPLES == 9
