"""numpy restatement of the VAE filter averaged over K posterior samples -- what csrc/p3d_vae_mc.h
is tested against.

For a row with encoder outputs mean, log_var and K draws eps_k, sample k is
y_k = decoder(eps_k exp(0.5 log_var) + mean) -- tests/vae_oracle.forward with eps_k, whose encoder
does not depend on eps -- and per output element

    m = y_0;  M = 0
    for k = 1 .. K - 1:   d = y_k - m;   m = m + d c_k;   M = M + d (y_k - m)
    y_mean = m            y_var = M c_{K-1}              c_j = (float)(1.0 / (double)(j + 1))

`fold` is that loop in float64 (c_j = 1 / (j + 1)) or in float32 with every operation rounded once
(the device's arithmetic word for word); `forward` runs it over vo.forward's samples, `filter` over
tests/vae_seq_oracle.filter's recurrence with the mean fed back.
"""
import numpy as np

import vae_oracle as vo
import vae_seq_oracle as so

MAX_K = 64


def c(j, dt=np.float32):
    """c_j: the float32 nearest to 1 / (j + 1) formed in double (float64: the quotient itself)."""
    q = 1.0 / float(j + 1)
    return np.float32(q) if dt == np.float32 else np.float64(q)


def fold(ys, dt=np.float64):
    """(y_mean, y_var) of the samples ys [K, ...] by the running fold, in `dt`."""
    ys = np.asarray(ys).astype(dt)
    K = ys.shape[0]
    assert 1 <= K <= MAX_K
    m = ys[0].copy()
    M = np.zeros_like(m)
    with np.errstate(invalid="ignore"):
        for k in range(1, K):
            d = ys[k] - m
            m = m + d * c(k, dt)
            M = M + d * (ys[k] - m)
        var = M * c(K - 1, dt)
    assert m.dtype == dt and var.dtype == dt
    return m, var


def forward(P, shape, x, eps, dt=np.float64):
    """eps [K, B, latent] -> {y, y_var, mean, log_var, ys [K, B, out]}."""
    cs = [vo.forward(P, shape, x, e, dt) for e in eps]
    ys = np.stack([k["y"] for k in cs])
    y, var = fold(ys, dt)
    return {"y": y, "y_var": var, "mean": cs[0]["mean"], "log_var": cs[0]["log_var"], "ys": ys}


def filter(P, shape, pred, seq_off, eps, target=None, state=None, dt=np.float64):
    """vae_seq_oracle.filter with r_f = the mean of K samples (eps [K, N, latent]) fed back.
    Returns {ref, ref_var, ys [K, N, out]} and, with a target, frame_err [N, 2] and seq_err [S, 2]."""
    out, L = shape[4], so.seq_len_of(shape)
    seq_off = np.asarray(seq_off, np.int64)
    eps = np.asarray(eps)
    K, S, N = eps.shape[0], len(seq_off) - 1, len(pred)
    assert seq_off[0] == 0 and seq_off[-1] == N and (np.diff(seq_off) >= 0).all()
    lens = np.diff(seq_off)
    pred = pred.astype(dt)
    ref, var = np.zeros((N, out), dt), np.zeros((N, out), dt)
    ys = np.zeros((K, N, out), dt)
    ferr = np.zeros((N, 2), dt)
    serr = np.zeros((S, 2), np.float64)
    buf = np.zeros((S, L * out), dt)
    for s in np.nonzero(lens > 0)[0]:
        if state is not None and state[1][s]:
            buf[s, out:] = state[0][s]
        else:
            buf[s] = np.tile(pred[seq_off[s]], L)
    for f in range(int(lens.max()) if S else 0):
        rows = np.nonzero(lens > f)[0]
        g = seq_off[rows] + f
        buf[rows] = np.concatenate([buf[rows, out:], pred[g]], axis=1)
        o = forward(P, shape, buf[rows], eps[:, g], dt)
        buf[rows, (L - 1) * out:] = o["y"]
        ref[g], var[g], ys[:, g] = o["y"], o["y_var"], o["ys"]
        if target is not None:
            t = target[g].astype(dt)
            ferr[g, 0] = np.mean(np.square(t - pred[g]), axis=-1, dtype=dt)
            ferr[g, 1] = np.mean(np.square(t - o["y"]), axis=-1, dtype=dt)
            serr[rows] += ferr[g].astype(np.float64)
    if state is not None:
        run = lens > 0
        state[0][run] = buf[run, out:]
        state[1][run] = 1
    res = {"ref": ref, "ref_var": var, "ys": ys}
    if target is not None:
        res["frame_err"], res["seq_err"] = ferr, serr
    return res


def var_bound(ys64, b):
    """The bound on |y_var - var_ref| that propagates from a per-sample forward bound: with
    var = c_{K-1} sum_k d_k^2 over the deviations d_k = y_k - mean, samples off by at most b move
    every d_k by at most 2 b (the sample and the mean), so d_k^2 by at most 4 b |d_k| + 4 b^2; the
    float32 fold's own rounding is covered by 1e-5 var_ref.  ys64 [K, ...]: the oracle's samples;
    b [...]: the largest forward bound over the K samples of each element."""
    ys64 = np.asarray(ys64, np.float64)
    K = ys64.shape[0]
    d = ys64 - ys64.mean(axis=0)
    var_ref = np.square(d).mean(axis=0)
    return (4.0 * b * np.abs(d) + 4.0 * b * b).sum(axis=0) / K + 1e-5 * var_ref
