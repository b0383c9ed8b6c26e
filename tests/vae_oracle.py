"""numpy restatement of the VAE pose filter (float64 and float32): forward, the three ELBO terms,
the analytic backward, Keras Adam and the eps stream -- what csrc/p3d_vae.h is tested against.

Reference: src/top_vae_3d_pose/models.py:12-91 (VAE), src/top_vae_3d_pose/losses.py:12-109 (ELBO)
and src/3d_pose_vae_filter.py:188-196 (train_step_vae).  The reference's own outputs need
TensorFlow 2 and are not available here; tests/test_vae_oracle.py pins this file against an
independent torch-autograd statement of the same graph instead.

A shape is (input_size, enc_dim tuple, latent_dim, dec_dim tuple, human_3d_size); parameters are a
dict under the Keras names, kernels [in, out], biases [out].
"""
import numpy as np

from oracle import ref_mlp

DEFAULT_SHAPE = (48, (40, 32), 24, (32, 40), 48)
# losses.py:74-75 after the reference's two decrements: bone a is joint a minus joint PARENT[a];
# a bone whose (once decremented) parent index is 0 is the joint itself (-1 here)
PARENT = (-1, 0, 1, -1, 3, 4, -1, 6, 7, 8, 7, 10, 11, 7, 13, 14)
EPS_SITE = 0x564145
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-7


def layer_names(shape):
    """[(keras layer name, K, N)] in creation order (models.py:25-52)."""
    n_in, enc, lat, dec, out = shape
    res, prev = [], n_in
    for u in enc:
        res.append(("enc_h_%d" % u, prev, u))
        prev = u
    res += [("mean", prev, lat), ("log_varianze", prev, lat)]
    prev = lat
    for u in dec:
        res.append(("dec_f_%d" % u, prev, u))
        prev = u
    res.append(("dec_f_out", prev, out))
    return res


def param_names(shape):
    """model.get_weights() order: kernel then bias of every layer."""
    return [(n + s, (K, N) if s == "/kernel" else (N,)) for n, K, N in layer_names(shape)
            for s in ("/kernel", "/bias")]


def init_params(shape, seed=0):
    """Glorot-uniform kernels, zero biases (keras.layers.Dense defaults)."""
    rng = np.random.default_rng(seed)
    P = {}
    for n, K, N in layer_names(shape):
        lim = np.sqrt(6.0 / (K + N))
        P[n + "/kernel"] = rng.uniform(-lim, lim, (K, N)).astype(np.float32)
        P[n + "/bias"] = np.zeros(N, np.float32)
    return P


def forward(P, shape, x, eps, dt=np.float64):
    """VAE.call with the caller's eps; returns a cache with every activation."""
    _, enc, lat, dec, _ = shape
    p = {k: v.astype(dt) for k, v in P.items()}
    h = x.astype(dt)
    c = {"enc_in": [], "dec_in": []}
    for u in enc:
        c["enc_in"].append(h)
        h = np.maximum(h @ p["enc_h_%d/kernel" % u] + p["enc_h_%d/bias" % u], dt(0))
    c["h"] = h
    c["mean"] = h @ p["mean/kernel"] + p["mean/bias"]
    c["log_var"] = h @ p["log_varianze/kernel"] + p["log_varianze/bias"]
    c["eps"] = eps.astype(dt)
    c["std"] = np.exp(dt(0.5) * c["log_var"])
    c["z"] = c["eps"] * c["std"] + c["mean"]
    dcur = c["z"]
    for u in dec:
        c["dec_in"].append(dcur)
        dcur = np.maximum(dcur @ p["dec_f_%d/kernel" % u] + p["dec_f_%d/bias" % u], dt(0))
    c["d"] = dcur
    c["y"] = dcur @ p["dec_f_out/kernel"] + p["dec_f_out/bias"]
    return c


def bones(y):
    """[B, 16, 3] bone directions of [B, 48] poses (losses.py:77-100)."""
    j = y.reshape(y.shape[0], 16, 3)
    b = j.copy()
    for a, par in enumerate(PARENT):
        if par >= 0:
            b[:, a] = j[:, a] - j[:, par]
    return b


def kcs_phi(y, t):
    bp, bt = bones(y), bones(t)
    return np.einsum("bac,bdc->bad", bp, bp) - np.einsum("bac,bdc->bad", bt, bt), bp


def row_terms(c, t, dt=np.float64):
    """[B, 3]: mean-square likelihood, KCS error (0 unless 48 outputs), KL (losses.py:29-32)."""
    t = t.astype(dt)
    y, mean, lv = c["y"], c["mean"], c["log_var"]
    like = np.mean(np.square(t - y), axis=-1, dtype=dt)
    kcs = np.abs(kcs_phi(y, t)[0]).sum(axis=(1, 2), dtype=dt) if y.shape[1] == 48 else np.zeros(len(y), dt)
    dkl = dt(0.5) * np.sum(np.exp(lv) + np.square(mean) - dt(1) - lv, axis=-1, dtype=dt)
    return np.stack([like, kcs, dkl], axis=1)


def loss3(terms, factors):
    """[likef mean_B like, kcsf mean_B kcs, dklf mean_B dkl] (losses.py:34-38)."""
    dt = terms.dtype.type
    return np.array([dt(f) * np.mean(terms[:, j], dtype=dt) for j, f in enumerate(factors)], dt)


def backward(P, shape, c, t, factors, dt=np.float64, trace=None):
    """Gradient of the three terms' sum w.r.t. every parameter; also returns dy.  `trace` (a list)
    receives (layer name, input activation, dz) of every dense layer."""
    _, enc, lat, dec, out = shape
    likef, kcsf, dklf = (dt(f) for f in factors)
    p = {k: v.astype(dt) for k, v in P.items()}
    t = t.astype(dt)
    B = dt(len(t))
    y = c["y"]
    dy = (dt(2) * likef / (B * dt(out))) * (y - t)
    if out == 48 and kcsf != 0:
        phi, bp = kcs_phi(y, t)
        s = np.sign(phi)
        db = dt(2) * np.einsum("bad,bdc->bac", s, bp)      # phi is symmetric: (S + S^T) bones
        dj = db.copy()
        for a, par in enumerate(PARENT):
            if par >= 0:
                dj[:, par] -= db[:, a]
        dy = dy + (kcsf / B) * dj.reshape(len(t), 48)
    g = {}

    def dense(name, a_in, dz):
        if trace is not None:
            trace.append((name, a_in, dz))
        g[name + "/kernel"] = a_in.T @ dz
        g[name + "/bias"] = dz.sum(axis=0, dtype=dt)
        return dz @ p[name + "/kernel"].T

    da = dense("dec_f_out", c["d"], dy)
    acts = c["dec_in"][1:] + [c["d"]]
    for u, a_in, a_out in reversed(list(zip(dec, c["dec_in"], acts))):
        da = dense("dec_f_%d" % u, a_in, da * (a_out > 0))
    ckl = dklf / B
    dmean = da + ckl * c["mean"]
    dlv = da * (dt(0.5) * (c["eps"] * c["std"])) + ckl * (dt(0.5) * (np.exp(c["log_var"]) - dt(1)))
    da = dense("mean", c["h"], dmean) + dense("log_varianze", c["h"], dlv)
    acts = c["enc_in"][1:] + [c["h"]]
    for u, a_in, a_out in reversed(list(zip(enc, c["enc_in"], acts))):
        da = dense("enc_h_%d" % u, a_in, da * (a_out > 0))
    return g, dy


def adam_init(P):
    return {"t": 0, "m": {k: np.zeros_like(v, np.float64) for k, v in P.items()},
            "v": {k: np.zeros_like(v, np.float64) for k, v in P.items()}}


def adam_apply(w, m, v, g, lr, t, dt=np.float64):
    """Keras Adam as TF2's fused apply, step t = 1, 2, ...: returns (w, m, v)."""
    lr_t = dt(lr) * np.sqrt(dt(1) - dt(BETA2) ** t) / (dt(1) - dt(BETA1) ** t)
    m = m + (g - m) * (dt(1) - dt(BETA1))
    v = v + (g * g - v) * (dt(1) - dt(BETA2))
    w = w - (lr_t * m) / (np.sqrt(v) + dt(ADAM_EPS))
    return w, m, v


def _u01(words):
    return ((words & np.uint32(0x7FFFFF)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)


def eps_stream(seed, ctr, row0, B, latent):
    """[B, latent] standard normals as k_vae_eps draws them: one Philox4x32-10 block per (row,
    column >> 2) under TF's Box-Muller.  The uint -> float conversions and the 2 pi u product are
    float32 like the kernel's; log, sqrt, sin and cos are float64 rounded to float32."""
    rows = (np.arange(B, dtype=np.int64) + row0).astype(np.uint32)[:, None]
    c4 = np.arange(latent // 4, dtype=np.uint32)[None, :]
    R, C = np.broadcast_arrays(rows, c4)
    w = ref_mlp.philox4x32_10(R, C, np.uint32(EPS_SITE), np.uint32(ctr & 0xFFFFFFFF), np.uint32(seed & 0xFFFFFFFF),
                              np.uint32((seed >> 32) & 0xFFFFFFFF))
    w = [np.asarray(x).astype(np.uint32) for x in w]
    out = np.empty((B, latent // 4, 4), np.float32)
    for h in range(2):
        u1 = np.maximum(_u01(w[2 * h]), np.float32(1e-7))
        ang = np.float32(6.28318530717958647692) * _u01(w[2 * h + 1])
        lg = np.log(u1.astype(np.float64)).astype(np.float32)
        r = np.sqrt((np.float32(-2.0) * lg).astype(np.float64)).astype(np.float32)
        out[:, :, 2 * h] = np.sin(ang.astype(np.float64)).astype(np.float32) * r
        out[:, :, 2 * h + 1] = np.cos(ang.astype(np.float64)).astype(np.float32) * r
    return out.reshape(B, latent)
