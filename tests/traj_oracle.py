"""numpy float64 oracle of the root trajectory (csrc/p3d_traj.h states the same
operations in the same order): per frame the camera-frame translation that puts the root-relative
3D joints of a `poses` row onto the 2D joints of an `xy_s` row under a pinhole camera, its
reprojection residual in pixels, and the windowed mean inside the clip.  Only + - * / and one sqrt,
every operation rounded on its own.

Rows are the clip calls': poses [N, 96] (32 joints, exported coordinates), xy_s [N, 36] (18 OpenPose
joints).  src holds row indices into the batch (-1: zeros), or None (every row its own).  Also the
synthetic rows the tests share (synth): a known translation, projected and written into both layouts."""
import numpy as np

from openpose_frontend import ORDER

JL = np.array([0, 1, 2, 3, 6, 7, 8, 17, 18, 19, 25, 26, 27])        # hip, legs, arms
NJ = len(JL)
D_MIN = 1e-12
MAX_HALF = 32
TOL = 1e-9
# the OpenPose joint of an H3.6M joint, from the frontend's own table; the hip is the mean of two
_OP = {h: i for i, h in enumerate(ORDER)}
OP_A = np.array([_OP[1] if j == 0 else _OP[j] for j in JL])         # the hip: RHip ...
OP_B = np.array([_OP[6] if j == 0 else _OP[j] for j in JL])         # ... and LHip


def fold16(v):
    """The fixed pairwise tree over 16 slots along the last axis (13 values and three +0.0): level 1
    adds slots 2i and 2i + 1, level 2 those results pairwise, and so on -- what an xor-butterfly
    over 16 lanes with d = 1, 2, 4, 8 yields, and what one lane adding in that order yields."""
    v = np.asarray(v, np.float64)
    s = np.zeros(v.shape[:-1] + (16,))
    s[..., :v.shape[-1]] = v
    while s.shape[-1] > 1:
        s = s[..., 0::2] + s[..., 1::2]
    return s[..., 0]


def joints_2d(xy_rows):
    """xy_s rows [N, 36] -> (u, v) [N, 13] of the 13 joints: the copied OpenPose joint, the hip as
    (RHip + LHip) / 2 (map_frames' form)."""
    xy = np.asarray(xy_rows, np.float64)
    ua, va, ub, vb = xy[:, 2 * OP_A], xy[:, 2 * OP_A + 1], xy[:, 2 * OP_B], xy[:, 2 * OP_B + 1]
    hip = JL == 0
    return np.where(hip, (ua + ub) / 2, ua), np.where(hip, (va + vb) / 2, va)


def joints_3d(poses):
    """poses rows [N, 96] -> root-relative camera coordinates (x, y, z) [N, 13] (the export's offsets cancel)."""
    P = np.asarray(poses, np.float64)
    x = P[:, 3 * JL] - P[:, 0:1]
    z = P[:, 3 * JL + 1] - P[:, 1:2]
    y = P[:, 2:3] - P[:, 3 * JL + 2]
    return x, y, z


def solve(poses, xy_s, src, focal, cx, cy):
    """-> traj_raw [N, 3], resid [N], valid [N] int32, D [N] (the denominators, for the tests' margin)."""
    poses, xy_s = np.asarray(poses, np.float64), np.asarray(xy_s, np.float64)
    N = poses.shape[0]
    s = np.arange(N) if src is None else np.asarray(src).astype(np.int64)
    zero = s < 0
    u, v = joints_2d(xy_s[np.clip(s, 0, N - 1)])
    x, y, z = joints_3d(poses)
    f = np.float64(focal)
    with np.errstate(all="ignore"):
        uc, vc = u - cx, v - cy
        a, b = uc / f, vc / f
        p, q = a * z - x, b * z - y
        am, bm, pm, qm = fold16(a) / NJ, fold16(b) / NJ, fold16(p) / NJ, fold16(q) / NJ
        da, db = a - am[:, None], b - bm[:, None]
        D = fold16(da * da + db * db)
        Nn = fold16(da * p + db * q)
        ok = ~zero & ~(D < D_MIN)                                     # (a NaN is not below the bound)
        Tz = -Nn / D
        Tx, Ty = pm + am * Tz, qm + bm * Tz
        Z = z + Tz[:, None]
        eu = f * ((x + Tx[:, None]) / Z) - uc
        ev = f * ((y + Ty[:, None]) / Z) - vc
        rs = np.sqrt(fold16(eu * eu + ev * ev) / NJ)
    T = np.where(ok[:, None], np.stack([Tx, Ty, Tz], axis=1), 0.0)
    return T, np.where(ok, rs, 0.0), ok.astype(np.int32), D


def smooth(raw, valid, off, h):
    """traj [N, 3]: per row the sum, in ascending order, of the valid raw rows at most h rows away
    inside the row's clip, over their number; zeros where the row is not valid.  h = 0: the raw rows."""
    raw = np.asarray(raw, np.float64)
    if h == 0:
        return raw.copy()
    out = np.zeros_like(raw)
    with np.errstate(all="ignore"):
        for c0, c1 in zip(off[:-1], off[1:]):
            for n in range(c0, c1):
                if not valid[n]:
                    continue
                acc, cnt = np.zeros(3), 0
                for m in range(max(c0, n - h), min(c1 - 1, n + h) + 1):
                    if valid[m]:
                        acc = acc + raw[m]
                        cnt += 1
                out[n] = acc / np.float64(cnt)
    return out


def trajectory(poses, xy_s, src, off, focal, cx, cy, h=0):
    """The whole call -> dict traj, traj_raw [N, 3], resid [N], valid [N] int32."""
    raw, rs, ok, _ = solve(poses, xy_s, src, focal, cx, cy)
    return {"traj": smooth(raw, ok, [int(o) for o in off], int(h)), "traj_raw": raw, "resid": rs, "valid": ok}


def close(got, want, what=""):
    """|got - want| <= 1e-9 max(1, |want|) everywhere, NaN exactly where want has NaN."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN in other places" % what
    err = np.abs(got - want)[~nan] / np.maximum(1.0, np.abs(want[~nan]))
    assert err.size == 0 or err.max() <= TOL, "%s: off by %.3e (relative to max(1, |value|))" % (what, err.max())
    return 0.0 if err.size == 0 else float(err.max())


# ---- the tests' synthetic rows -----------------------------------------------------------------
F, CX, CY = 1145.0, 512.0, 515.0          # H3.6M's nominal camera


def synth(n, seed, spine=True):
    """n rows with a known translation: joints N(0, 300 mm) around a zero hip, Tx in +-1500, Ty in
    +-800, Tz in [2000, 8000], projected with (F, CX, CY) -> (poses [n, 96] in exported layout with
    the export's offsets, xy_s [n, 36] in OpenPose order through the inverse of ORDER, T [n, 3]).  The
    left hip is moved sideways so that the two 2D hips' mean is the hip's projection.  The joints the
    solve does not use hold other values (NaN in the 3D row's unused joints when spine=False)."""
    rng = np.random.default_rng(seed)
    J = rng.normal(0.0, 300.0, (n, 32, 3))                            # camera frame (x, y, z)
    J[:, 0] = 0.0
    T = np.stack([rng.uniform(-1500, 1500, n), rng.uniform(-800, 800, n), rng.uniform(2000, 8000, n)], axis=1)
    C = J + T[:, None, :]
    # the 2D hip is the mean of the two 2D hips (map_frames): the left hip (joint 6) keeps its drawn
    # depth and moves sideways to where its projection mirrors the right hip's about the hip's
    for k in (0, 1):
        m = 2 * (C[:, 0, k] / C[:, 0, 2]) - C[:, 1, k] / C[:, 1, 2]
        C[:, 6, k] = m * C[:, 6, 2]
    J = C - T[:, None, :]
    u, v = F * C[..., 0] / C[..., 2] + CX, F * C[..., 1] / C[..., 2] + CY
    xy = rng.uniform(100.0, 900.0, (n, 18, 2))                        # joints the mapping does not read: anything
    for i, h in enumerate(ORDER):
        xy[:, i, 0], xy[:, i, 1] = u[:, h], v[:, h]
    ox, oz = rng.uniform(-300, 300, (n, 1)), rng.uniform(-300, 300, (n, 1))   # the export's offsets
    P = np.stack([J[..., 0] + ox, J[..., 2] + 3000.0, -J[..., 1] + oz], axis=-1)
    if not spine:
        unused = np.setdiff1d(np.arange(32), JL)
        P[:, unused] = np.nan
    return P.reshape(n, 96), xy.reshape(n, 36), T


def lstsq_T(poses_row, xy_row, focal, cx, cy):
    """The same translation from np.linalg.lstsq on the stacked 26 x 3 system."""
    u, v = joints_2d(xy_row[None])
    x, y, z = joints_3d(poses_row[None])
    a, b = (u[0] - cx) / focal, (v[0] - cy) / focal
    A = np.zeros((2 * NJ, 3))
    A[:NJ, 0], A[:NJ, 2] = 1.0, -a
    A[NJ:, 1], A[NJ:, 2] = 1.0, -b
    rhs = np.concatenate([a * z[0] - x[0], b * z[0] - y[0]])
    return np.linalg.lstsq(A, rhs, rcond=None)[0]
