"""The live tick planner (csrc/p3d_live_plan.h) through p3d_live_plan, without a GPU: which frames
of which slots become final in a tick is a pure function of the per-slot counts and the tick's push
and close masks.  A schedule of streams -- lengths 1, 2, 8, 9, 10 and 13, opened at different ticks,
with ticks in which a slot is skipped and slots reused after close -- is driven tick by tick and
every stream's concatenated rows are checked against the rule."""
import ctypes
import os
import sys

import numpy as np
import pytest

import _p3d

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import live_oracle  # noqa: E402

NONE, HEAD, MIDDLE, TAIL = 0, 1, 2, 3


class Planner:
    def __init__(self, S, smooth=1):
        self.S, self.smooth = S, smooth
        self.count = np.zeros(S, np.int32)
        self.off = np.zeros(S + 1, np.int64)
        self.slot, self.frame, self.kind = (np.full(5 * S, -9, np.int32) for _ in range(3))
        self.push_frame, self.short = np.zeros(S, np.int32), np.zeros(S, np.int32)

    def tick(self, push=(), close=()):
        """-> ({slot: [(frame, kind)]}, push_frame, short slots), or the error message."""
        pm, cm = np.zeros(self.S, np.uint8), np.zeros(self.S, np.uint8)
        pm[list(push)] = 1
        cm[list(close)] = 1
        n = ctypes.c_int64(-1)
        d = lambda a: a.ctypes.data   # noqa: E731
        rc = _p3d.lib().p3d_live_plan(self.S, self.smooth, d(self.count), d(pm), d(cm), d(self.off), d(self.slot),
                                      d(self.frame), d(self.kind), d(self.push_frame), d(self.short), ctypes.byref(n))
        if rc:
            assert rc == _p3d.P3D_ERR_ARG
            return _p3d.lib().p3d_last_error().decode()
        N = int(n.value)
        assert self.off[0] == 0 and self.off[self.S] == N and (np.diff(self.off) >= 0).all() and N <= 5 * self.S
        rows = {}
        for s in range(self.S):
            a, b = int(self.off[s]), int(self.off[s + 1])
            assert (self.slot[a:b] == s).all()
            if b > a:
                rows[s] = list(zip(self.frame[a:b].tolist(), self.kind[a:b].tolist()))
        return rows, self.push_frame.copy(), set(np.flatnonzero(self.short).tolist())


def schedule():
    """(slot, first tick, length, ticks skipped) per stream; slots 0 and 2 are reused after close."""
    return [(0, 0, 13, {4, 9}), (1, 2, 9, set()), (2, 0, 1, set()), (3, 5, 10, {7}), (2, 3, 8, {5}),
            (0, 20, 2, set()), (2, 16, 9, {17, 18}), (1, 14, 1, set())]


def drive(smooth):
    """Run the schedule; per stream -> dict(rows [(tick, frame, kind)], pushes [tick of frame f], closed, short)."""
    pl = Planner(4, smooth)
    streams = [dict(slot=sl, t0=t0, n=n, skip=skip, sent=0, rows=[], pushes=[], closed=None, short=False)
               for sl, t0, n, skip in schedule()]
    for tick in range(40):
        push, close = {}, {}
        for st in streams:
            if st["closed"] is not None or tick < st["t0"]:
                continue
            if st["sent"] == st["n"]:
                close[st["slot"]] = st
            elif tick not in st["skip"]:
                push[st["slot"]] = st
        assert not set(push) & set(close)
        if not push and not close:
            continue
        rows, push_frame, short = pl.tick(push, close)
        for s in range(4):
            assert push_frame[s] == (push[s]["sent"] if s in push else -1)
        for sl, st in push.items():
            st["pushes"].append(tick)
            st["sent"] += 1
        for sl, st in close.items():
            st["closed"], st["short"] = tick, sl in short
            assert pl.count[sl] == 0                                  # the slot starts from nothing again
        assert short <= set(close)
        for sl, r in rows.items():
            st = push.get(sl) or close[sl]
            st["rows"] += [(tick, f, k) for f, k in r]
        assert set(rows) <= set(push) | set(close)
    assert all(st["closed"] is not None for st in streams)
    return streams


def test_every_frame_once_in_order_with_the_right_window_and_in_time():
    streams = drive(1)
    assert sorted(st["n"] for st in streams) == [1, 1, 2, 8, 9, 9, 10, 13]
    for st in streams:
        n, rows = st["n"], st["rows"]
        if 2 <= n <= 8:
            assert st["short"] and rows == []                        # reported, nothing emitted
            continue
        assert not st["short"]
        assert [f for _, f, _ in rows] == list(range(n))             # exactly once, in order
        for tick, f, k in rows:
            want = NONE if n == 1 else HEAD if f < 4 else TAIL if f >= n - 4 else MIDDLE
            assert k == want, (n, f, k)
            if f >= n - 4:                                           # the last four (and a single frame): at close
                assert tick == st["closed"]
            else:                                                    # no later than four pushes after its own
                assert tick == st["pushes"][max(f + 4, 8)]
        if n == 9:
            assert [f for _, f, k in rows if k == MIDDLE] == [4]
        per_tick = {}
        for tick, _, _ in rows:
            per_tick[tick] = per_tick.get(tick, 0) + 1
        assert set(per_tick.values()) <= {1, 4, 5}
        # the numpy restatement of the rule gives the same table
        frames, kinds, _ = live_oracle.run_stream(np.ones((n, 36)))
        assert frames == [f for _, f, _ in rows] and kinds == [k for _, _, k in rows]


def test_without_smoothing_every_frame_is_final_at_once():
    for st in drive(0):
        assert not st["short"]
        assert st["rows"] == [(t, f, NONE) for f, t in enumerate(st["pushes"])]


def test_argument_errors():
    pl = Planner(4)
    msg = pl.tick(push=(1,), close=(1,))
    assert msg.startswith("p3d_live_plan: ") and "slot 1" in msg and "pushed and closed" in msg
    assert (pl.count == 0).all()
    lib = _p3d.lib()
    n = ctypes.c_int64()
    a = ctypes.c_void_p(pl.count.ctypes.data)
    assert lib.p3d_live_plan(0, 1, a, a, a, a, a, a, a, a, a, ctypes.byref(n)) == _p3d.P3D_ERR_ARG
    assert b"S must be" in lib.p3d_last_error()
    assert lib.p3d_live_plan(4, 1, a, a, a, a, None, a, a, a, a, ctypes.byref(n)) == _p3d.P3D_ERR_ARG
    assert b"null" in lib.p3d_last_error()
    pl.count[2] = -1
    assert "slot 2" in pl.tick(push=(2,))
