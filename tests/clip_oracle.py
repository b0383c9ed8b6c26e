"""CPU oracle for a whole OpenPose clip (src/openpose_3dpose_sandbox.py).  TEST INFRASTRUCTURE ONLY.

A numpy restatement, written from the definition (not from the reference's text), of

* ``smooth``: read_openpose_json's median windows and the hold of dropped joints (:140-227);
* ``post``: the per-frame axis swap, flip and spine offset (:366-383) and --cache_on_fail
  (:389-417) applied to the unnormalised [N, 96] poses.

``smooth`` is pinned bit for bit to the reference's own function by
tests/golden/clip_goldens.npz (tests/test_clip_host.py).  All arithmetic is float64.
"""
from __future__ import annotations

import numpy as np


def _median(window):
    """np.median of the window's values put in order by a STABLE sort (the reference sorts with
    Python's sorted(): among equal values, -0.0 == 0.0 included, the window order stays), [W, 36]
    -> [36].  Seven values: the middle one; four: (a + b) / 2 of the two middle ones.  A NaN
    anywhere in a column's window gives NaN."""
    w = np.asarray(window, np.float64)
    s = np.sort(w, axis=0, kind="stable")
    n = s.shape[0]
    with np.errstate(invalid="ignore"):
        med = s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2
    return np.where(np.isnan(w).any(axis=0), np.nan, med)


def smooth(xy, smooth=True):
    """xy [N, 36] in position order -> the smoothed, held rows [N, 36]."""
    xy = np.array(xy, np.float64)
    n = xy.shape[0]
    if not smooth or n == 1:
        return xy
    if n <= 8:
        raise ValueError("need more frames, min 9 frames for smoothing")
    out = np.empty_like(xy)
    for i in range(n):
        if i < 4:                       # the window's order: the frame itself, then outwards
            rows = [i, i + 1, i + 2, i + 3]
        elif i >= n - 4:
            rows = [i, i - 1, i - 2, i - 3]
        else:
            rows = [i, i + 1, i + 2, i + 3, i - 1, i - 2, i - 3]
        med = _median(xy[rows])
        if i > 0:
            med = np.where(med == 0.0, out[i - 1], med)      # the hold (NaN != 0: kept)
        out[i] = med
    return out


def post(unnorm, xy_s, cache_on_fail=True):
    """unnorm [N, 96] (unNormalizeData's rows), xy_s [N, 36] -> (poses [N, 96], src [N] int32)."""
    un = np.asarray(unnorm, np.float64)
    n = un.shape[0]
    poses = np.zeros((n, 96))
    src = np.full(n, -1, np.int32)
    before, before_src = None, -1
    for f in range(n):
        p = un[f].reshape(32, 3).copy()
        p[:, [1, 2]] = p[:, [2, 1]]                           # swap y and z
        _max, _min = 0.0, 10000.0
        for z in p[:, 2]:
            if z > _max:
                _max = z
            if z < _min:
                _min = z
        spine_x, spine_y = xy_s[f, 2], xy_s[f, 3]
        with np.errstate(invalid="ignore", over="ignore"):
            p[:, 2] = (_max - p[:, 2]) + _min
            p[:, 0] = p[:, 0] + (spine_x - 630)
            p[:, 2] = p[:, 2] + (500 - spine_y)
        row, row_src = p.reshape(96), f
        if cache_on_fail:
            if np.min(row) < -1000:                           # (a NaN minimum compares False)
                row, row_src = before, before_src
            before, before_src = row, row_src
        if row is not None:
            poses[f], src[f] = row, row_src
    return poses, src


def unnormalize(y, mean3, std3, use3):
    """unNormalizeData (src/data_utils.py:283-311) of float32 rows y [N, U3] -> [N, 96] float64."""
    y = np.asarray(y, np.float32)
    orig = np.zeros((y.shape[0], 96), np.float32)
    orig[:, np.asarray(use3)] = y
    return orig * np.asarray(std3, np.float64)[None, :] + np.asarray(mean3, np.float64)[None, :]
