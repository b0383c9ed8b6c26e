"""Golden vectors for the spline resampling, made with scipy: the reference's
``--interpolation`` stage (src/openpose_3dpose_sandbox.py:252-266) fits every smoothed track with

    spl = UnivariateSpline(frame, x, k=3)
    spl.set_smoothing_factor(float((max(x) - min(x)) * 125))
    xnew = spl(np.arange(0, framerange, multiplier))

Run by hand where scipy is installed (nothing on the GPU machine imports scipy):

    python tests/golden/make_golden_spline.py

Output: tests/golden/spline_goldens.npz -- per curve ``y_<i>`` (the track), ``t1_<i>`` / ``c1_<i>``
(knots and coefficients after the constructor), ``t_<i>`` / ``c_<i>`` (after set_smoothing_factor),
``v<R>_<i>`` = spl(np.arange(0, m, 1.0 / R)) for R in 1, 2, 10, ``fresh_<i>`` (the coefficients of a
fresh UnivariateSpline(s=S): what the continuation is not) and the table ``meta`` [curves, 10]:
m, n1, ier1, n, ier2, branch (0 A .. 3 D, 4 a non-finite sample), fp1, fp, S, fp0.  Inputs and recorded results only.

The tracks are of the kinds a clip holds: smooth motion with detector noise (a joint that moves, one
that hardly moves), the jumpy median-filtered-and-held kind of tests/golden/clip_goldens.npz, a zero
run at the clip's start (a joint first seen late, as parsed with smoothing off), a constant column (a
joint never seen) and a column with one NaN sample."""
import os
import sys

import numpy as np
from scipy.interpolate import UnivariateSpline

HERE = os.path.dirname(os.path.abspath(__file__))
MS = (4, 5, 9, 23, 64, 129, 300)
RS = (1, 2, 10)
BRANCH = {"A": 0, "B": 1, "C": 2, "D": 3, "N": 4}            # N: a non-finite sample, no branch claimed


def smooth_track(rng, m, amp, noise=1.0):
    x = np.arange(m)
    ph = rng.uniform(0, 6.28, 2)
    return 600.0 + amp * np.sin(x * 0.07 + ph[0]) + 0.3 * amp * np.sin(x * 0.31 + ph[1]) + noise * rng.standard_normal(m)


def jumpy_track(rng, m):
    """make_clip_golden.synth's kind after the hold: uniform positions, each kept for a few frames."""
    v = rng.uniform(40.0, 900.0, m)
    keep = rng.random(m) < 0.45
    keep[0] = True
    return v[np.maximum.accumulate(np.where(keep, np.arange(m), 0))]


def tracks():
    """(name, y) for every golden curve, the same on every run."""
    rng = np.random.default_rng(20251021)
    out = []
    for m in MS:
        out.append(("move_%d" % m, smooth_track(rng, m, 50.0)))
        out.append(("move2_%d" % m, smooth_track(rng, m, 80.0, 2.0)))
        out.append(("still_%d" % m, smooth_track(rng, m, 0.01)))
        out.append(("jumpy_%d" % m, jumpy_track(rng, m)))
        y = smooth_track(rng, m, 60.0)
        y[:max(1, m // 4)] = 0.0
        out.append(("zerorun_%d" % m, y))
    out.append(("const_23", np.full(23, 311.5)))
    out.append(("const_64", np.zeros(64)))
    y = smooth_track(rng, 23, 40.0)
    y[7] = np.nan
    out.append(("nan_23", y))
    for seed in range(1000, 3000):                            # a curve on which FITPACK reports ier > 0 (3: 20 iterations)
        y = jumpy_track(np.random.default_rng(seed), 27)
        f = fit(y)
        if f["ier1"] > 0 and f["ier2"] > 0:
            out.append(("ier3_27", y))
            break
    for m in (600, 1000, 2000):                               # Branch C: a joint that hardly moves in a long clip
        out.append(("lowmotion_%d" % m, smooth_track(rng, m, 1.0)))
    return out


def fit(y):
    m = len(y)
    x = [float(v) for v in y]
    spl = UnivariateSpline(range(m), x, k=3)
    d = spl._data
    n1, ier1, fp1 = int(d[7]), int(d[-1]), float(d[10])
    t1, c1 = d[8][:n1].copy(), d[9][:n1].copy()
    fp0 = float(d[11][n1 - 1])
    S = float((max(x) - min(x)) * 125)
    spl.set_smoothing_factor(S)
    d = spl._data
    n, ier2, fp = int(d[7]), int(d[-1]), float(d[10])
    t, c = d[8][:n].copy(), d[9][:n].copy()
    if S == 0.0:
        branch = "D"
    elif not np.isfinite(x).all():
        branch = "N"
    elif n1 == 8 or S >= fp0:
        branch = "A"
    else:
        branch = "C" if n > n1 else "B"
    vals = {}
    for R in RS:
        at = np.arange(0, m, 1.0 / R)
        assert len(at) == R * m, (m, R, len(at))
        vals[R] = spl(at)
    fresh = UnivariateSpline(range(m), x, k=3, s=S)._data if S == S else None
    return dict(m=m, n1=n1, ier1=ier1, fp1=fp1, t1=t1, c1=c1, n=n, ier2=ier2, fp=fp, t=t, c=c, S=S, fp0=fp0,
                branch=branch, vals=vals, fresh=None if fresh is None else fresh[9][:int(fresh[7])].copy())


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    import spline_oracle as so
    out, meta, names = {}, [], []
    c_curve = None
    for name, y in tracks():
        f = fit(y)
        if name.startswith("lowmotion"):                      # keep the shortest that reaches Branch C
            if f["branch"] != "C" or c_curve is not None:
                continue
            c_curve = name
        i = len(names)
        names.append(name)
        out["y_%d" % i] = np.asarray(y, np.float64)
        for k in ("t1", "c1", "t", "c"):
            out["%s_%d" % (k, i)] = f[k]
        for R in RS:
            out["v%d_%d" % (R, i)] = f["vals"][R]
        if f["fresh"] is not None:
            out["fresh_%d" % i] = f["fresh"]
        meta.append([f["m"], f["n1"], f["ier1"], f["n"], f["ier2"], BRANCH[f["branch"]], f["fp1"], f["fp"], f["S"], f["fp0"]])
        o = so.fit(y)
        print("%-14s m %4d  n1 %4d ier1 %2d  n %4d ier2 %2d  branch %s  oracle margin %.2e at %s"
              % (name, f["m"], f["n1"], f["ier1"], f["n"], f["ier2"], f["branch"], o["margin"], o["margin_at"]))
    out["meta"] = np.array(meta, np.float64)
    out["names"] = np.array(names)
    path = os.path.join(HERE, "spline_goldens.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; ier > 0 curves:", [n for n, r in zip(names, meta) if r[2] > 0 or r[4] > 0])


if __name__ == "__main__":
    main()
