"""The denoiser's sample sets: the numeric half of gen_sample_img (src/vae_filter.py:22-46).

The reference picks nine test poses, runs their noised versions through encode, reparametrize and
decode, un-normalises the real, the noised and the predicted poses and draws them.  gen_samples
returns (and optionally saves) those three sets; the drawing itself is not part of this package,
which does not depend on a plotting library.
"""
import os

import numpy as np

import data_utils

NSAMPLES = 9


def _rows(a, idx):
    """Rows idx of a numpy array or a (device) tensor."""
    if isinstance(a, np.ndarray):
        return a[idx, :]
    import torch
    return a[torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(a.device)]


def _host(a):
    return a if isinstance(a, np.ndarray) else a.detach().cpu().numpy()


def gen_samples(model, real, noised, mean, std, dim_ignored, idx=None, nsamples=NSAMPLES, path=None):
    """`nsamples` rows of real / noised [n, d] (numpy or device tensors) un-normalised to [nsamples, D]
    float64, and, with a model, the filter's prediction for them:
    pred = decode(reparametrize(*encode(noised[idx]))).  idx: the rows, else drawn as the reference
    draws them, np.random.choice(n, nsamples, replace=False).  Returns {"idx", "real", "noised"} and,
    with a model, "pred"; with `path` the same arrays are saved as one .npz."""
    n = int(real.shape[0])
    if tuple(noised.shape) != tuple(real.shape):
        raise ValueError("gen_samples: real is %s, noised is %s" % (tuple(real.shape), tuple(noised.shape)))
    if idx is None:
        idx = np.random.choice(n, nsamples, replace=False)
    idx = np.asarray(idx, dtype=np.int64)
    if idx.ndim != 1 or idx.size < 1 or idx.min() < 0 or idx.max() >= n:
        raise ValueError("gen_samples: idx must be a vector of rows in 0 .. %d" % (n - 1))
    real_points, noised_points = _rows(real, idx), _rows(noised, idx)
    out = {"idx": idx}
    if model is not None:
        z = model.reparametrize(*model.encode(noised_points))
        pred_points = model.decode(z)
    out["real"] = data_utils.unNormalizeData(_host(real_points), mean, std, dim_ignored)
    out["noised"] = data_utils.unNormalizeData(_host(noised_points), mean, std, dim_ignored)
    if model is not None:
        out["pred"] = data_utils.unNormalizeData(_host(pred_points), mean, std, dim_ignored)
    if path is not None:
        np.savez(path if str(path).endswith(".npz") else str(path) + ".npz", **out)
    return out


def sample_path(samples_dir, epoch):
    """Where vae_filter.train writes an epoch's sample set."""
    return os.path.join(samples_dir, "samples_%04d.npz" % epoch)
