"""CPU oracle for live OpenPose streams (csrc/p3d_live_plan.h, csrc/p3d_live.h).  TEST INFRASTRUCTURE ONLY.

A numpy restatement of the streaming state machine, one ``Stream`` per live stream: the emission
rule (which frames become final at a push and at close), the ring of raw frames the window medians
read, the hold from the stream's last smoothed row and the last good pose of --cache_on_fail.  It
is written as recurrences with the state the kernels carry -- nothing of it looks at a frame list
as a whole -- so that feeding it tick by tick and comparing with ``clip_oracle`` on the whole stream
shows that the streaming contract IS the clip's contract (tests/test_live_oracle.py).
"""
from __future__ import annotations

import numpy as np

import clip_oracle

NONE, HEAD, MIDDLE, TAIL = 0, 1, 2, 3
RING = 16
WINDOW = {NONE: (0,), HEAD: (0, 1, 2, 3), TAIL: (0, -1, -2, -3), MIDDLE: (0, 1, 2, 3, -1, -2, -3)}


def plan_push(n, smooth=True):
    """The rows [(frame, kind)] that become final when a stream receives its n-th frame."""
    if not smooth:
        return [(n - 1, NONE)]
    if n == 9:
        return [(f, HEAD) for f in range(4)] + [(4, MIDDLE)]
    return [(n - 5, MIDDLE)] if n > 9 else []


def plan_close(n, smooth=True):
    """The rows that become final when a stream of n frames is closed (ValueError: 2 .. 8 frames)."""
    if not smooth or n == 0:
        return []
    if n == 1:
        return [(0, NONE)]
    if n <= 8:
        raise ValueError("need more frames, min 9 frames for smoothing")
    return [(f, TAIL) for f in range(n - 4, n)]


class Stream:
    """One live stream's carried state: n, the ring, the last smoothed row, the last good pose."""

    def __init__(self, smooth=True, cache_on_fail=True):
        self.smooth, self.cache = bool(smooth), bool(cache_on_fail)
        self.n = 0
        self.ring = np.zeros((RING, 36))
        self.last = np.zeros(36)
        self.good, self.good_pos = None, -1

    def _smooth_row(self, f, kind):
        med = clip_oracle._median(self.ring[[(f + k) % RING for k in WINDOW[kind]]]) if kind != NONE else self.ring[f % RING].copy()
        if kind != NONE and f > 0:
            med = np.where(med == 0.0, self.last, med)       # the hold (NaN != 0: kept); never at frame 0
        self.last = med
        return med

    def push(self, xy):
        """A new raw frame -> [(frame, kind, xy_s row)] that became final."""
        self.ring[self.n % RING] = np.asarray(xy, np.float64)
        self.n += 1
        return [(f, k, self._smooth_row(f, k)) for f, k in plan_push(self.n, self.smooth)]

    def close(self):
        rows = [(f, k, self._smooth_row(f, k)) for f, k in plan_close(self.n, self.smooth)]
        self.n = 0
        return rows

    def finish(self, frame, unnorm_row, xy_s_row):
        """One row's post-processing with the carried last good pose -> (pose [96], src)."""
        pose = clip_oracle.post(np.asarray(unnorm_row)[None, :], np.asarray(xy_s_row)[None, :], cache_on_fail=False)[0][0]
        if self.cache and np.min(pose) < -1000:              # (a NaN minimum compares False)
            return (self.good.copy(), self.good_pos) if self.good is not None else (np.zeros(96), -1)
        self.good, self.good_pos = pose, frame
        return pose.copy(), frame


def run_stream(xy, smooth=True):
    """A whole stream pushed frame by frame and closed -> (frames, kinds, xy_s rows) in emission order."""
    st = Stream(smooth)
    rows = []
    for row in xy:
        rows += st.push(row)
    rows += st.close()
    return ([f for f, _, _ in rows], [k for _, k, _ in rows],
            np.array([r for _, _, r in rows]).reshape(len(rows), 36))
