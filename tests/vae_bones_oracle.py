"""numpy restatement of the bones filter (float64 and float32): the decoder topology, the four row
terms, the loss 4-vector, the analytic backward and the joints <-> bones conversions -- what the
bones kind of csrc/p3d_vae.h and csrc/p3d_bones.h are tested against.

Reference: src/top_vae_3d_pose/models.py:544-573 (VAEBones), src/top_vae_3d_pose/losses.py:113-156
(loss_bones), src/top_vae_3d_pose/bones.py:71-153.  tests/test_vae_bones_oracle.py pins this file
against an independent torch-autograd statement of the graph and against the reference's own
conversions (tests/golden/bones_goldens.npz).

A shape is (input_size, enc_dim tuple, latent_dim, dec_dim tuple); the output is always 64 =
[mag (16) | cos (16 x 3)].  The decoder ends dec_dim -> mag1 (16, ReLU) -> {mag2 (16), cos2 (48)}:
both linear heads read mag1's output (models.py:559-566).  The reference's layer cos1 is
overwritten before keras.Model is formed, is not reachable from the outputs and has no weights.
"""
import numpy as np

import vae_oracle as vo

DEFAULT_SHAPE = (1376, (40, 32), 24, (32, 40))
BJA = np.array([0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 9, 14, 15, 9, 11, 12])      # bones.py:74
BJB = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 14, 15, 16, 11, 12, 13])   # bones.py:75


def layer_names(shape):
    """[(keras layer name, K, N)]: the VAE's table up to dec_f_<units>, then mag1, mag2, cos2."""
    n_in, enc, lat, dec = shape
    res = vo.layer_names((n_in, enc, lat, dec, 48))[:-1]
    return res + [("mag1", dec[-1], 16), ("mag2", 16, 16), ("cos2", 16, 48)]


def param_names(shape):
    return [(n + s, (K, N) if s == "/kernel" else (N,)) for n, K, N in layer_names(shape)
            for s in ("/kernel", "/bias")]


def init_params(shape, seed=0):
    rng = np.random.default_rng(seed)
    P = {}
    for n, K, N in layer_names(shape):
        lim = np.sqrt(6.0 / (K + N))
        P[n + "/kernel"] = rng.uniform(-lim, lim, (K, N)).astype(np.float32)
        P[n + "/bias"] = np.zeros(N, np.float32)
    return P


def forward(P, shape, x, eps, dt=np.float64):
    """VAEBones.call with the caller's eps; `y` is [B, 64] = [mag2's output | cos2's output]."""
    n_in, enc, lat, dec = shape
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
    c["m1"] = np.maximum(c["d"] @ p["mag1/kernel"] + p["mag1/bias"], dt(0))
    c["mag"] = c["m1"] @ p["mag2/kernel"] + p["mag2/bias"]
    c["cos"] = c["m1"] @ p["cos2/kernel"] + p["cos2/bias"]
    c["y"] = np.concatenate([c["mag"], c["cos"]], axis=1)
    return c


def gram(cosines):
    """[B, 16, 16]: G[a][b] = cos[a] . cos[b] of [B, 48] cosine rows (losses.py:147-151)."""
    v = cosines.reshape(len(cosines), 16, 3)
    return np.einsum("bac,bdc->bad", v, v)


def row_terms(c, t, dt=np.float64):
    """[B, 4]: mean_16 (tm - pm)^2, 3 mean_48 (tc - pc)^2, KL, mean_16x16 |G(tc) - G(pc)|."""
    t = t.astype(dt)
    tm, tc = t[:, :16], t[:, 16:]
    mag = np.mean(np.square(tm - c["mag"]), axis=-1, dtype=dt)
    cos = dt(3) * np.mean(np.square(tc - c["cos"]), axis=-1, dtype=dt)
    dkl = dt(0.5) * np.sum(np.exp(c["log_var"]) + np.square(c["mean"]) - dt(1) - c["log_var"], axis=-1, dtype=dt)
    ang = np.abs(gram(tc) - gram(c["cos"])).sum(axis=(1, 2), dtype=dt) / dt(256)
    return np.stack([mag, cos, dkl, ang], axis=1)


def loss4(terms, factors):
    """[magf mean_B MAG, cosf mean_B COS, dklf mean_B DKL, angf mean_B ANG] (losses.py:143-154)."""
    dt = terms.dtype.type
    return np.array([dt(f) * np.mean(terms[:, j], dtype=dt) for j, f in enumerate(factors)], dt)


def backward(P, shape, c, t, factors, dt=np.float64, trace=None):
    """Gradient of the four terms' sum w.r.t. every parameter; also returns dy [B, 64]."""
    _, enc, lat, dec = shape
    magf, cosf, dklf, angf = (dt(f) for f in factors)
    p = {k: v.astype(dt) for k, v in P.items()}
    t = t.astype(dt)
    B = dt(len(t))
    tm, tc = t[:, :16], t[:, 16:]
    dmag = (dt(2) * magf / (dt(16) * B)) * (c["mag"] - tm)
    phi = gram(c["cos"]) - gram(tc)
    pc = c["cos"].reshape(len(t), 16, 3)
    dang = dt(2) * np.einsum("bad,bdc->bac", np.sign(phi), pc)      # phi is symmetric
    dcos = (angf / (dt(256) * B)) * dang.reshape(len(t), 48) + (cosf / (dt(8) * B)) * (c["cos"] - tc)
    dy = np.concatenate([dmag, dcos], axis=1)
    g = {}

    def dense(name, a_in, dz):
        if trace is not None:
            trace.append((name, a_in, dz))
        g[name + "/kernel"] = a_in.T @ dz
        g[name + "/bias"] = dz.sum(axis=0, dtype=dt)
        return dz @ p[name + "/kernel"].T

    da = dense("mag2", c["m1"], dmag) + dense("cos2", c["m1"], dcos)
    da = dense("mag1", c["d"], da * (c["m1"] > 0))
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


# ------------------------------------------------------------------ joints <-> bones
def bones_from_joints(joints, dt=np.float64):
    """[B, 48] float32 -> [B, 64] float32 = [mag | cos].  dt = float64: convert_to_bones
    (bones.py:101-121: float64 arithmetic, one rounding at the end); dt = float32:
    convert_to_bones_tf (bones.py:71-98) with the sum of squares taken left to right."""
    j = np.concatenate([np.zeros((len(joints), 3), dt), np.asarray(joints, np.float32).astype(dt)], axis=1)
    j = j.reshape(len(joints), 17, 3)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = j[:, BJB] - j[:, BJA]
        sq = v * v
        mag = np.sqrt((sq[:, :, 0] + sq[:, :, 1]) + sq[:, :, 2])
        cos = v / mag[:, :, None]
    assert mag.dtype == dt and cos.dtype == dt
    return np.concatenate([mag, cos.reshape(len(joints), 48)], axis=1).astype(np.float32)


def bones_to_joints(bones64):
    """[B, 64] float32 -> float64 [B, 48]: in bone order J[BJB] = J[BJA] + float64(cos *_32 mag)
    (bones.py:124-153)."""
    b = np.asarray(bones64, np.float32)
    mag, cos = b[:, :16], b[:, 16:].reshape(len(b), 16, 3)
    J = np.zeros((len(b), 17, 3), np.float64)
    for k in range(16):
        prod = cos[:, k] * mag[:, k, None]
        assert prod.dtype == np.float32
        J[:, BJB[k]] = J[:, BJA[k]] + prod
    return J[:, 1:].reshape(len(b), 48)
