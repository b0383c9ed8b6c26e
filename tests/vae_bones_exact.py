"""Integer-valued bones filters: forward, ANG term and EVERY gradient without a tolerance (the idea
of tests/vae_exact.py carried to the bones kind of csrc/p3d_vae.h).

Weights are 0 / +-1 (two non-zeros per column), biases small integers, the log_varianze layer all
zero (log_var = 0, std = 1, no KL gradient on log_var), the inputs small integers, the caller's eps
even integers and the targets the exact outputs plus small integers.  The factors make every
coefficient exact: mag = 8 B (2 mag / (16 B) = 1), cos = 8 B (cos / (8 B) = 1), dkl = B (dkl / B =
1), ang = 8 B (ang / (256 B) = 2^-5).  Then y, mean and z are integers, the ANG row term an
integer over 256, and every gradient a multiple of UNIT = 2^-5; exact_case proves, per case, that
the float32 and float64 oracles agree bit for bit, that every gradient is a whole number of units
below 2^24 and that the sum of absolute values of every contraction stays below 2^23 units -- so
any summation order, tiling or launch form gives these bits.

The MAG, COS and KL row terms and the loss 4-vector are NOT exact (a division by 16, 48, B): they
stay with the tolerance tests.
"""
import numpy as np

import vae_bones_oracle as vb

UNIT = 2.0 ** -5
LIMIT = 2.0 ** 23
_cache = {}


def integer_params(shape, seed=11, nnz=2):
    rng = np.random.default_rng(seed)
    P = {}
    for n, K, N in vb.layer_names(shape):
        w = np.zeros((K, N), np.float32)
        if n != "log_varianze":
            for j in range(N):
                rows = rng.choice(K, size=min(nnz, K), replace=False)
                w[rows, j] = rng.choice([-1.0, 1.0], size=len(rows))
        P[n + "/kernel"] = w
        P[n + "/bias"] = (np.zeros(N, np.float32) if n == "log_varianze"
                          else rng.integers(-1, 2, size=N).astype(np.float32))
    return P


def factors_for(B):
    return (8.0 * B, 8.0 * B, float(B), 8.0 * B)


def _abs_sums(P, c, trace, t):
    """The largest sum of absolute values of every contraction of forward, ANG term and backward."""
    a = {k: np.abs(v.astype(np.float64)) for k, v in P.items()}
    worst = {}
    for name, a_in, dz in trace:
        ai, adz = np.abs(a_in), np.abs(dz) / UNIT
        worst[name] = max(float((ai @ a[name + "/kernel"] + a[name + "/bias"]).max()),   # forward
                          float((ai.T @ adz).max()), float(adz.sum(axis=0).max()),      # dW, db
                          float((adz @ a[name + "/kernel"].T).max()))                   # da
    # the two heads are one packed layer on the device: its data gradient sums over all 64 columns
    tr = {n: (ai, dz) for n, ai, dz in trace}
    worst["out"] = float((np.abs(tr["mag2"][1]) / UNIT @ a["mag2/kernel"].T
                          + np.abs(tr["cos2"][1]) / UNIT @ a["cos2/kernel"].T).max())
    ap, at = np.abs(c["cos"]), np.abs(t[:, 16:].astype(np.float64))
    psi = vb.gram(ap) + vb.gram(at)
    worst["ang"] = max(float(psi.sum(axis=(1, 2)).max()),
                       float(8.0 * ap.reshape(len(ap), 16, 3).sum(axis=1).max() + (ap + at).max() / UNIT))
    return worst


def exact_case(B, shape):
    """{P, x, t, eps, factors, y, mean, z, ang, grads} of the integer case at batch B, proven exact;
    computed once per process and shared (read-only arrays)."""
    key = (B, shape)
    if key in _cache:
        return _cache[key]
    P = integer_params(shape)
    rng = np.random.default_rng(2000 + B)
    x = rng.integers(-2, 3, size=(B, shape[0])).astype(np.float32)
    eps = (2 * rng.integers(-1, 2, size=(B, shape[2]))).astype(np.float32)
    factors = factors_for(B)
    y0 = vb.forward(P, shape, x, eps, np.float64)["y"]
    t = (y0 + rng.integers(-2, 3, size=y0.shape)).astype(np.float32)
    res = {}
    for dt in (np.float32, np.float64):
        c = vb.forward(P, shape, x, eps, dt)
        trace = []
        g, _ = vb.backward(P, shape, c, t, factors, dt, trace=trace)
        res[dt] = (c, g, vb.row_terms(c, t, dt)[:, 3], trace)
    (c, g, ang, _), (c64, g64, ang64, trace64) = res[np.float32], res[np.float64]
    for k in ("y", "mean", "z", "log_var"):
        assert c[k].dtype == np.float32 and np.array_equal(c[k], c64[k]), "%s differs between float32 and float64" % k
        assert np.array_equal(c[k], np.round(c[k])), "%s is not an integer" % k
    assert not c["log_var"].any()
    assert ang.dtype == np.float32 and np.array_equal(ang, ang64) and np.array_equal(256 * ang, np.round(256 * ang))
    assert ang.any()
    assert sorted(g) == sorted(n for n, _ in vb.param_names(shape))
    for name, v in g.items():
        assert v.dtype == np.float32, name
        assert np.array_equal(v, g64[name]), "%s differs between float32 and float64" % name
        units = g64[name] / UNIT
        assert np.array_equal(units, np.round(units)), "%s is not a whole number of units" % name
        assert float(np.abs(units).max()) < 2.0 ** 24, "%s is not representable" % name
    assert any(v.any() for v in g.values())
    worst = _abs_sums(P, c64, trace64, t)
    for name, w in worst.items():
        assert w < LIMIT, "%s: a contraction's absolute sum %g leaves float32's exact range" % (name, w)
    out = {"P": P, "x": x, "t": t, "eps": eps, "factors": factors, "y": c["y"], "mean": c["mean"], "z": c["z"],
           "ang": ang, "grads": g, "worst": worst}
    for v in [x, t, eps, c["y"], c["mean"], c["z"], ang, *g.values(), *P.values()]:
        v.setflags(write=False)
    _cache[key] = out
    return out
