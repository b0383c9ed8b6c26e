"""The root trajectory's definition (tests/traj_oracle.py), checked on the CPU: the
closed form recovers a known translation, agrees with a generic least-squares solve, and the special
rows and the smoothing window behave as stated."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import traj_oracle as to   # noqa: E402

DRAWS = 2000


def _rel(got, T):
    """The error relative to the translation's length: a component may lie anywhere near zero (Tx, Ty
    are drawn around it), and its error is set by Tz's, not by its own size."""
    return np.abs(got - T).max(axis=1) / np.sqrt((T * T).sum(axis=1))


def _solved():
    P, xy, T = to.synth(DRAWS, seed=11)
    raw, rs, ok, D = to.solve(P, xy, None, to.F, to.CX, to.CY)
    return P, xy, T, raw, rs, ok, D


def test_fold16_is_the_pairwise_tree():
    v = np.random.default_rng(0).standard_normal(13) * 10.0 ** np.arange(13)
    s = list(v) + [0.0] * 3
    lvl1 = [s[2 * i] + s[2 * i + 1] for i in range(8)]
    lvl2 = [lvl1[2 * i] + lvl1[2 * i + 1] for i in range(4)]
    want = (lvl2[0] + lvl2[1]) + (lvl2[2] + lvl2[3])
    assert to.fold16(v) == want
    # the butterfly: every lane ends with the same bits
    lanes = np.array(s)
    for d in (1, 2, 4, 8):
        lanes = lanes + lanes[np.arange(16) ^ d]
    assert (lanes == want).all()


def test_recovers_the_translation_and_agrees_with_lstsq():
    P, xy, T, raw, rs, ok, D = _solved()
    assert ok.all() and ok.dtype == np.int32
    # the margin: no row is anywhere near the degenerate branch, and 1 / D amplifies rounding by at
    # most 1e4 -- a few dozen roundings of 1.1e-16 stay orders below the 1e-9 asked for
    assert D.min() > 1e-4, D.min()
    rel = _rel(raw, T)
    assert rel.max() <= 1e-9, rel.max()
    assert rs.max() < 1e-6, rs.max()
    worst = 0.0
    for n in range(0, DRAWS, 4):
        ref = to.lstsq_T(P[n], xy[n], to.F, to.CX, to.CY)
        worst = max(worst, to.close(raw[n], ref, "lstsq row %d" % n))
    print("min D %.3e, worst |T - T0| / |T0| %.3e, worst resid %.3e px, worst lstsq disagreement %.3e"
          % (D.min(), rel.max(), rs.max(), worst))


def test_unused_joints_are_not_read():
    P, xy, T = to.synth(50, seed=3, spine=False)                      # NaN in every 3D joint outside the 13
    raw, rs, ok, _ = to.solve(P, xy, None, to.F, to.CX, to.CY)
    assert ok.all() and np.isfinite(raw).all() and _rel(raw, T).max() <= 1e-9


def test_special_rows():
    P, xy, T = to.synth(12, seed=5)
    src = np.arange(12, dtype=np.int32)
    xy[3] = np.tile([400.0, 300.0], 18)                               # all 2D joints equal: degenerate
    src[5] = -1                                                       # a zero row
    src[7] = 6                                                        # a held row: shows row 6's pose
    P[7] = P[6]
    xy[7] = 0.0                                                       # its own detections are what failed
    P[9, 3 * 7 + 1] = np.nan                                          # a NaN joint among the 13
    raw, rs, ok, D = to.solve(P, xy, src, to.F, to.CX, to.CY)
    assert D[3] < to.D_MIN
    for n in (3, 5):
        assert ok[n] == 0 and rs[n] == 0.0 and not raw[n].any() and not np.signbit(raw[n]).any()
    assert ok[7] == 1 and raw[7].tobytes() == raw[6].tobytes() and rs[7] == rs[6]
    assert ok[9] == 1 and np.isnan(raw[9]).all() and np.isnan(rs[9])
    rest = [0, 1, 2, 4, 6, 8, 10, 11]
    assert _rel(raw[rest], T[rest]).max() <= 1e-9
    # a null src: every row its own
    raw0, _, ok0, _ = to.solve(P, xy, None, to.F, to.CX, to.CY)
    assert ok0[5] == 1 and raw0[[0, 1, 2]].tobytes() == raw[[0, 1, 2]].tobytes()


def test_smoothing_windows():
    rng = np.random.default_rng(2)
    off = [0, 1, 3, 10, 30]
    raw = rng.standard_normal((30, 3)) * 1000.0
    valid = np.ones(30, np.int32)
    valid[[4, 12, 13, 29]] = 0
    raw[valid == 0] = 0.0
    assert to.smooth(raw, valid, off, 0).tobytes() == raw.tobytes()   # h = 0: the raw bytes
    for h in (1, 4, 32):
        out = to.smooth(raw, valid, off, h)
        for c0, c1 in zip(off[:-1], off[1:]):
            for n in range(c0, c1):
                lo, hi = max(c0, n - h), min(c1 - 1, n + h)
                rows = [m for m in range(lo, hi + 1) if valid[m]]
                if not valid[n]:
                    assert not out[n].any()
                    continue
                acc = np.zeros(3)
                for m in rows:
                    acc = acc + raw[m]
                assert out[n].tobytes() == (acc / len(rows)).tobytes(), (h, n)
        assert out[0].tobytes() == raw[0].tobytes()                   # a one-frame clip: itself
        # a clip alone has the bits it has inside the batch
        alone = to.smooth(raw[10:30], valid[10:30], [0, 20], h)
        assert alone.tobytes() == out[10:30].tobytes()
    # a window never crosses a clip end: changing a neighbouring clip changes nothing
    other = raw.copy()
    other[3:10] += 5.0
    a, b = to.smooth(raw, valid, off, 32), to.smooth(other, valid, off, 32)
    assert a[:3].tobytes() == b[:3].tobytes() and a[10:].tobytes() == b[10:].tobytes()


def test_trajectory_puts_the_pieces_together():
    P, xy, T = to.synth(20, seed=8)
    r = to.trajectory(P, xy, None, [0, 9, 20], to.F, to.CX, to.CY, 0)
    assert r["traj"].tobytes() == r["traj_raw"].tobytes() and r["valid"].all()
    r4 = to.trajectory(P, xy, None, [0, 9, 20], to.F, to.CX, to.CY, 4)
    assert r4["traj_raw"].tobytes() == r["traj_raw"].tobytes()
    to.close(r4["traj"][0], r["traj_raw"][0:5].mean(axis=0), "the first row's window")
