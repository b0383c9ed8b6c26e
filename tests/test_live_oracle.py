"""The streaming state machine (tests/live_oracle.py: ring, hold, last good pose), fed tick by tick,
equals tests/clip_oracle.py on the whole stream bit for bit: the live contract is the clip's
contract.  No GPU, no library."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import clip_oracle  # noqa: E402
import live_oracle  # noqa: E402


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok], b[ok]) and np.array_equal(np.signbit(a[ok]), np.signbit(b[ok]))


def crafted_stream(n, seed):
    """Raw frames with dropped joints (zeros) in runs from frame 0 and across every tick, -0.0
    medians (at frame 0: kept with its sign; later: held) and a NaN."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(40.0, 900.0, (n, 36))
    xy[rng.random((n, 36)) < 0.3] = 0.0
    xy[:, 0] = 0.0                                   # dropped from frame 0 on: stays zero
    xy[:, 1:8] = rng.uniform(40.0, 900.0, (n, 7))
    if n >= 9:
        xy[0:7, 1] = 0.0                             # dropped from frame 0 over the head rows, then seen
        xy[3:n - 2, 2] = 0.0                         # a run across (nearly) every tick, ending before the tail
        xy[n - 6:, 3] = 0.0                          # a run into the tail rows
        xy[n // 2, 4] = np.nan                       # a NaN: not zero, kept
        xy[2:8, 5] = -0.0                            # -0.0 medians past frame 0: held
        xy[0:6, 6] = -0.0                            # a -0.0 median AT frame 0: kept with its sign
    return xy


@pytest.mark.parametrize("n", [1, 9, 10, 13, 16, 17, 40])
def test_smoothing_tick_by_tick_equals_the_clip(n):
    xy = crafted_stream(n, 100 + n)
    frames, kinds, got = live_oracle.run_stream(xy, smooth=True)
    want = clip_oracle.smooth(xy, smooth=True)
    assert frames == list(range(n))
    assert same_bits(got, want)
    if n >= 9:
        # the cases are really there (properties of the clip oracle's result alone)
        assert not want[:, 0].any()
        assert want[0, 6] == 0 and np.signbit(want[0, 6])
        assert np.isnan(want[:, 4]).any()
        assert n < 13 or want[3, 2] == want[4, 2] == want[5, 2] != 0   # held across the ticks
        assert kinds[:5] == [1, 1, 1, 1, 2] and kinds[-4:] == [3] * 4


@pytest.mark.parametrize("n", [1, 5, 12])
def test_without_smoothing_every_frame_passes_through_at_once(n):
    xy = crafted_stream(n, 7 + n)
    st = live_oracle.Stream(smooth=False)
    for i, row in enumerate(xy):
        out = st.push(row)
        assert [(f, k) for f, k, _ in out] == [(i, live_oracle.NONE)]
        assert same_bits(out[0][2], row)
    assert st.close() == []


@pytest.mark.parametrize("n", [2, 5, 8])
def test_short_streams_are_refused_at_close(n):
    st = live_oracle.Stream()
    for row in crafted_stream(n, n):
        assert st.push(row) == []
    with pytest.raises(ValueError, match="min 9 frames"):
        st.close()


@pytest.mark.parametrize("cache", [True, False])
@pytest.mark.parametrize("lead", [0, 1, 6])
def test_last_good_pose_row_by_row_equals_the_clip(cache, lead):
    """Failing runs from frame 0 (zeros, -1), across ticks and of a whole one-frame stream."""
    rng = np.random.default_rng(3 + lead)
    for n in (1, 13, 20):
        un = rng.uniform(-900, 900, (n, 96))
        xy_s = rng.uniform(400, 700, (n, 36))
        fail = np.zeros(n, bool)
        fail[:min(lead, n)] = True
        if n >= 13:
            fail[8:12] = True
            un[7, 5] = np.nan                                  # a NaN minimum: kept
        un[fail, 0] = -5000.0
        want, want_src = clip_oracle.post(un, xy_s, cache_on_fail=cache)
        st = live_oracle.Stream(cache_on_fail=cache)
        got = [st.finish(f, un[f], xy_s[f]) for f in range(n)]
        assert same_bits(np.array([g[0] for g in got]), want)
        assert [g[1] for g in got] == list(want_src)
        if cache and lead:
            assert want_src[0] == -1 and not want[0].any()
