"""numpy restatement of the device noise stream (csrc/p3d_vae_noise.h, include/p3d.h
p3d_vae_add_noise) -- what k_vae_noise is tested against -- and the four statistics both it and the
host add_noise are held to.

Built on oracle/ref_mlp.philox4x32_10 and on vae_oracle's Box-Muller: `normals4` below is
vae_oracle.eps_stream's construction with the site as an argument (vae_oracle._u01, float32
conversions and 2 pi u product, log / sqrt / sin / cos in float64 rounded to float32);
tests/test_vae_noise_oracle.py pins it to eps_stream bit for bit at the eps site.
"""
import math

import numpy as np

import vae_oracle as vo
from oracle import ref_mlp

NOISE_SITE = 0x4E4F49
NOISE_ROW_SITE = 0x4E4F52
THRESHOLD = 0xB103AF11
NOISE = 0.22108747
NOISE_OFFSET = 0.0011787938
P_NOISED = 1.0 - 0.5 * (1.0 + math.erf(0.5 / math.sqrt(2.0)))     # 1 - Phi(0.5) = 0.3085...


def _philox(rows, c4, site, seed, ctr):
    R, C = np.broadcast_arrays(np.asarray(rows, np.uint32), np.asarray(c4, np.uint32))
    w = ref_mlp.philox4x32_10(R, C, np.uint32(site), np.uint32(ctr & 0xFFFFFFFF), np.uint32(seed & 0xFFFFFFFF),
                              np.uint32((seed >> 32) & 0xFFFFFFFF))
    return [np.asarray(x).astype(np.uint32) for x in w]


def normals4(rows, c4, site, seed, ctr):
    """[..., 4] float32: the four normals of the Philox blocks (rows, c4, site, ctr), key seed."""
    w = _philox(rows, c4, site, seed, ctr)
    out = np.empty(w[0].shape + (4,), np.float32)
    for h in range(2):
        u1 = np.maximum(vo._u01(w[2 * h]), np.float32(1e-7))
        ang = np.float32(6.28318530717958647692) * vo._u01(w[2 * h + 1])
        lg = np.log(u1.astype(np.float64)).astype(np.float32)
        r = np.sqrt((np.float32(-2.0) * lg).astype(np.float64)).astype(np.float32)
        out[..., 2 * h] = np.sin(ang.astype(np.float64)).astype(np.float32) * r
        out[..., 2 * h + 1] = np.cos(ang.astype(np.float64)).astype(np.float32) * r
    return out


def row_decisions(B, width, seed, ctr, row0=0):
    """(mask [B] bool: the noised rows, jid [B]: the chosen joint's first column) of rows row0 ..
    row0 + B - 1 -- row block A alone, integers only."""
    g = (np.arange(B, dtype=np.int64) + row0).astype(np.uint32)      # (the low 32 bits)
    A = _philox(g, np.zeros(B, np.uint32), NOISE_ROW_SITE, seed, ctr)
    mask = A[0] >= np.uint32(THRESHOLD)
    jc = ((A[1].astype(np.uint64) * np.uint64(width)) >> np.uint64(32)).astype(np.int64)
    return mask, jc - jc % 3


def noise_stream(x, seed, ctr, row0=0, noise=NOISE, offset=NOISE_OFFSET, joint_scale=None, noise_3d=(1, 1)):
    """The noised copy of x [B, width] float32 as p3d_vae_add_noise forms it for rows row0 .. row0 +
    B - 1.  Returns (out, mask [B] bool: the noised rows, jid [B]: the chosen joint's first column
    (of every row, noised or not), e [B, width]: the element normals, j [B, 3]: the joint's)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, width = x.shape
    assert width % 12 == 0
    noise, offset = np.float32(noise), np.float32(offset)
    joint_scale = np.float32(NOISE + noise_3d[1]) if joint_scale is None else np.float32(joint_scale)
    g = (np.arange(B, dtype=np.int64) + row0).astype(np.uint32)
    e = normals4(g[:, None], np.arange(width // 4, dtype=np.uint32)[None, :], NOISE_SITE, seed, ctr).reshape(B, width)
    mask, jid = row_decisions(B, width, seed, ctr, row0)
    j = normals4(g, np.ones(B, np.uint32), NOISE_ROW_SITE, seed, ctr)[:, :3]
    out = x.copy()
    rows = np.nonzero(mask)[0]
    out[rows] = x[rows] + (e[rows] * noise + offset)                 # float32, each operation rounded once
    for k in range(3):
        out[rows, jid[rows] + k] = out[rows, jid[rows] + k] + j[rows, k] * joint_scale
    return out, mask, jid, e, j


def statistics(x, out, noise_3d=(1, 1), jid=None):
    """The four statistics of a noised copy as z scores (deviation from the exact value over the
    estimator's standard error) under the model: a row is noised with probability 1 - Phi(0.5); a
    noised row's difference is width independent N(OFFSET, NOISE^2) plus three N(0, (NOISE +
    noise_3d[1])^2) on one uniformly chosen joint.

    A row counts as noised iff it differs from x.  The chosen joint is `jid` // 3 where the caller
    knows it (the stream's own); otherwise (the host add_noise, which does not return it) the joint
    with the largest squared difference: when the chosen joint's three normals are all small another
    joint wins, and which one is uniform over the others and independent of the choice, so the
    histogram's model -- every bin Binomial(m, 1 / joints) -- holds either way."""
    d = np.asarray(out, np.float64) - np.asarray(x, np.float64)
    n, width = d.shape
    s2, off, sj2 = NOISE ** 2, NOISE_OFFSET, (NOISE + noise_3d[1]) ** 2
    mask = np.any(np.asarray(out) != np.asarray(x), axis=1)
    m = int(mask.sum())
    dn = d[mask]
    z = {"share": (m / n - P_NOISED) / math.sqrt(P_NOISED * (1 - P_NOISED) / n)}
    # row sum: width N(off, s2) + 3 N(0, sj2)
    z["sum"] = (dn.sum(axis=1).mean() - width * off) / math.sqrt((width * s2 + 3 * sj2) / m)
    # row sum of squares: (width - 3) elements N(off, s2) and 3 elements N(off, s2 + sj2);
    # Var(X^2) = 2 v^2 + 4 mu^2 v for X ~ N(mu, v)
    var_sq = lambda mu, v: 2 * v * v + 4 * mu * mu * v               # noqa: E731
    mean_sq = width * (s2 + off ** 2) + 3 * sj2
    var_row = (width - 3) * var_sq(off, s2) + 3 * var_sq(off, s2 + sj2)
    z["sumsq"] = (np.square(dn).sum(axis=1).mean() - mean_sq) / math.sqrt(var_row / m)
    joints = width // 3
    pick = (np.square(dn).reshape(m, joints, 3).sum(axis=2).argmax(axis=1) if jid is None
            else np.asarray(jid)[mask] // 3)
    hist = np.bincount(pick, minlength=joints)
    p = 1.0 / joints
    z["joint"] = float(np.abs(hist - m * p).max() / math.sqrt(m * p * (1 - p)))
    return z, m
