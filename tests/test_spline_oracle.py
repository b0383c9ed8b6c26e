"""tests/spline_oracle.py (the arithmetic csrc/p3d_spline.h restates) against scipy's
FITPACK as recorded in tests/golden/spline_goldens.npz (make_golden_spline.py): the reference's
UnivariateSpline(frame, y, k=3) then set_smoothing_factor((max - min) * 125), sampled at
np.arange(0, m, 1 / R).

n, ier and every knot (frame indices: whole numbers) must be equal.  Coefficients and samples are
compared as |d| / max(1, max y - min y).  MEASURED is the largest such value over the golden set on
the machine that made the goldens (MEASUREMENTS.md 30): 0.0 -- the oracle's operation order is the
Fortran's and that build contracts nothing, so every coefficient and sample carries scipy's bits --
and the bound is 16 times that: equality.  Only curves whose decision margins exceed 1e-6 take part
(closer to a decision two correct arithmetics may branch differently); at most one in ten may be left
out and every branch must keep a curve."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import spline_oracle as so  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "spline_goldens.npz"))
NAMES = [str(n) for n in GOLD["names"]]
META = GOLD["meta"]                                           # m, n1, ier1, n, ier2, branch, fp1, fp, S, fp0
RS = (1, 2, 10)
MEASURED = 0.0
BOUND = 16 * MEASURED
MARGIN = 1e-6
BRANCHES = {0: "A", 1: "B", 2: "C", 3: "D"}

_FITS = {}


def fit(i):
    if i not in _FITS:
        _FITS[i] = so.fit(GOLD["y_%d" % i])
    return _FITS[i]


def finite(i):
    return bool(np.isfinite(GOLD["y_%d" % i]).all())


def taking_part():
    return [i for i in range(len(NAMES)) if finite(i) and fit(i)["margin"] > MARGIN]


def test_the_golden_set_reaches_every_case():
    br = META[:, 5].astype(int)
    assert set(BRANCHES) <= set(br.tolist())
    assert sorted({int(m) for m in META[:, 0]} & {4, 5, 9, 23, 64, 129, 300}) == [4, 5, 9, 23, 64, 129, 300]
    assert (META[:, 2] == -2).any()                                          # a stage-1 polynomial
    assert any(n.startswith("zerorun") for n in NAMES) and any(n.startswith("const") for n in NAMES)
    assert any(not finite(i) for i in range(len(NAMES)))                     # a NaN sample
    assert ((META[:, 2] > 0) | (META[:, 4] > 0)).any()                       # ier > 0: the iteration limit
    c = [i for i in range(len(NAMES)) if br[i] == 2]
    assert c and all(META[i, 3] > META[i, 1] for i in c)                     # Branch C adds knots in stage 2
    part = taking_part()
    left_out = sum(finite(i) for i in range(len(NAMES))) - len(part)
    assert 10 * left_out <= len(NAMES), "%d curves within %g of a decision" % (left_out, MARGIN)
    for b, name in BRANCHES.items():
        assert any(br[i] == b for i in part), "no Branch %s curve takes part" % name


@pytest.mark.parametrize("i", range(len(NAMES)), ids=NAMES)
def test_fit_equals_scipy(i):
    if i not in taking_part():                                # (a non-finite sample: test_nan_mask; or too close to a
        return                                                # decision: counted in test_the_golden_set_reaches_every_case)
    f = fit(i)
    m, n1, ier1, n, ier2 = (int(v) for v in META[i, :5])
    assert (f["n1"], f["ier1"], f["n"], f["ier2"]) == (n1, ier1, n, ier2)
    np.testing.assert_array_equal(f["t1"], GOLD["t1_%d" % i])
    np.testing.assert_array_equal(f["t"], GOLD["t_%d" % i])
    assert (f["t"] == np.round(f["t"])).all()
    y = GOLD["y_%d" % i]
    scale = max(1.0, float(y.max() - y.min()))
    worst = max(np.abs(f["c1"][:n1 - 4] - GOLD["c1_%d" % i][:n1 - 4]).max(),
                np.abs(f["c"][:n - 4] - GOLD["c_%d" % i][:n - 4]).max()) / scale
    for R in RS:
        want = GOLD["v%d_%d" % (R, i)]
        got = so.splev(f["t"], f["c"], np.arange(R * m, dtype=np.float64) * (1.0 / R))
        assert got.shape == want.shape == (R * m,)
        worst = max(worst, np.abs(got - want).max() / scale)
    print("%s: |d| / max(1, range) = %.3e" % (NAMES[i], worst))
    assert worst <= BOUND, worst


def test_nan_mask():
    """A column holding a NaN follows the arithmetic: scipy's NaN mask, sample for sample."""
    for i in range(len(NAMES)):
        if finite(i):
            continue
        f = fit(i)
        m = int(META[i, 0])
        assert (f["n1"], f["ier1"], f["n"], f["ier2"]) == tuple(int(v) for v in META[i, 1:5])
        np.testing.assert_array_equal(f["t"], GOLD["t_%d" % i])
        np.testing.assert_array_equal(np.isnan(f["c"][:f["n"] - 4]), np.isnan(GOLD["c_%d" % i][:f["n"] - 4]))
        for R in RS:
            got = so.splev(f["t"], f["c"], np.arange(R * m, dtype=np.float64) * (1.0 / R))
            np.testing.assert_array_equal(np.isnan(got), np.isnan(GOLD["v%d_%d" % (R, i)]))


def test_count_and_extrapolated_tail():
    i = NAMES.index("move_23")
    y = GOLD["y_%d" % i]
    for R in (2, 10):
        f = so.resample(y, R)
        assert f["xr"].shape == (R * 23,)
        t, c, n = f["t"], f["c"], f["n"]
        assert t[n - 4] == 22.0                                              # xe: the samples beyond it extrapolate
        tail = np.arange(R * 22 + 1, R * 23, dtype=np.float64) * (1.0 / R)
        assert tail.size == R - 1 and (tail > 22.0).all()
        # the last polynomial piece, continued: its cubic through four of its own samples inside the interval
        lo = t[n - 5]
        xs = np.linspace(lo, 22.0, 4)
        poly = np.polyfit(xs - 22.0, so.splev(t, c, xs), 3)
        np.testing.assert_allclose(f["xr"][R * 22 + 1:], np.polyval(poly, tail - 22.0), rtol=1e-9)


def test_stage_two_continues_stage_one():
    """set_smoothing_factor(S) is not a fresh fit with s = S: on a Branch B curve the two differ."""
    i = NAMES.index("move_300")
    assert int(META[i, 5]) == 1
    y = GOLD["y_%d" % i]
    f, fresh = fit(i), so.fresh_fit(y, META[i, 8])
    np.testing.assert_array_equal(fresh["c"][:fresh["n"] - 4], GOLD["fresh_%d" % i][:fresh["n"] - 4])   # scipy's fresh fit
    at = np.arange(300, dtype=np.float64)
    d = np.abs(so.splev(f["t"], f["c"], at) - so.splev(fresh["t"], fresh["c"], at)).max()
    assert fresh["n"] != f["n"] and d > 0.5, (fresh["n"], f["n"], d)


def test_span_factor_is_pythons_min_max():
    y = [3.0, float("nan"), 7.0, -1.0]
    assert so.span_factor(y) == (max(y) - min(y)) * 125.0 == 1000.0
    y = [float("nan"), 1.0, 2.0]
    assert np.isnan(so.span_factor(y)) and np.isnan((max(y) - min(y)) * 125.0)
