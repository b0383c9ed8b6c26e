"""k_serve6_rounds with helper waves (csrc/p3d_serve6_helpers.h): a long launch's contraction waves
never stop between blocks; four helper waves do the K-combine, epilogue, stores, posts, the next
round's input layers and the previous round's output tiles.

The helpers keep the 256-thread form's tile dealing, slice order and clamped duplicates, so every
launch must have the BITS of
  * the same launch on a model created under P3D_SERVE6_HELPERS=0 (k_serve6_rounds_w4: one wave per
    SIMD, each doing its own boundary work), and
  * the same rows served one round (1,280 rows) per launch by the 20-step kernel,
and the fp64 oracle's values within 2e-5 + 2e-5 |ref|.

Shapes: the narrowest and the widest the form takes (L = 768: 12 k-groups per wave -- three ring
rounds, nothing between the post and the flag request -- and members with one or two tiles; L =
1,024), one block (four blocks per round: the input-layer boundaries follow the output boundary at
once, and the epilogue that rewrites slab 3 is the block after the output tiles) and two.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import _p3d  # noqa: E402
import exact_models  # noqa: E402
import linear_model  # noqa: E402
from oracle import ref_mlp  # noqa: E402

ROUND = 1280
HELPERS = "k_serve6_rounds<4, 3, 2, 5>"
PARENT = "k_serve6_rounds_w4<4, 3, 2, 5>"
SHORT = "k_serve6<4, 3, 2, 5, true>"


def model(cfg, st):
    m = linear_model.LinearModel(cfg.linear_size, cfg.num_layers, cfg.residual, cfg.batch_norm, cfg.max_norm,
                                 64, 1e-3, "/tmp/p3d_test", cfg.predict_14, seed=11, max_batch=64)
    m.set_weights({**st.params, **st.moving})
    return m


def kname(m):
    name = _p3d.ctypes.create_string_buffer(128)
    _p3d.check(_p3d.lib().p3d_kernel_name(m._h, 3, name, 128), "p3d_kernel_name")
    return name.value.decode()


def close(a, b, atol=2e-5, rtol=2e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b)
    tol = atol + rtol * np.abs(b)
    assert np.all(err <= tol), "max err %.3g (at ref %.3g)" % (err.max(), b.flat[np.argmax(err - tol)])


def chunked(m, xd):
    """The rows of xd served one round (1,280 rows) per launch: the 20-step kernel on whole rounds."""
    out = []
    for i in range(0, xd.shape[0], ROUND):
        out.append(m.serve_device(xd[i:i + ROUND]))
        if xd.shape[0] - i >= ROUND:
            assert kname(m) == SHORT, kname(m)
    return torch.cat(out)


_models = {}


@pytest.fixture(scope="module")
def models(request):
    """(state, helper-form model, parent-form model) per (L, blocks), made once."""
    def get(L, N):
        if (L, N) not in _models:
            cfg = ref_mlp.Cfg(linear_size=L, num_layers=N, residual=True, batch_norm=True)
            st = ref_mlp.init_state(cfg, seed=L + N, bn_seed=2)
            mp = pytest.MonkeyPatch()
            mh = model(cfg, st)
            mp.setenv("P3D_SERVE6_HELPERS", "0")
            m4 = model(cfg, st)
            mp.undo()
            _models[(L, N)] = (st, mh, m4)
        return _models[(L, N)]
    yield get
    for _, mh, m4 in _models.values():
        mh.close()
        m4.close()
    _models.clear()


def check_launch(st, mh, m4, B, oracle_idx=None):
    x = np.random.default_rng(B).standard_normal((B, 32)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    y = mh.serve_device(xd)
    assert kname(mh) == HELPERS, kname(mh)
    y4 = m4.serve_device(xd)
    assert kname(m4) == PARENT, kname(m4)
    yc = chunked(mh, xd)
    torch.cuda.synchronize()
    mh.serve_check()
    m4.serve_check()
    assert not bool(torch.isnan(y).any())
    assert torch.equal(y, y4), "rows differ from the one-wave-per-SIMD form: %d" % int((y != y4).any(dim=1).sum())
    assert torch.equal(y, yc), "rows differ from the 20-step launches: %d" % int((y != yc).any(dim=1).sum())
    idx = np.arange(B) if oracle_idx is None else oracle_idx
    ro, _ = ref_mlp.forward(st, x[idx], False, 1.0, 0, 0, 0)
    close(y.cpu().numpy()[idx], ro)


@pytest.mark.parametrize("B", [
    33 * 64 + 1,      # 2,113: a ragged second round -- groups with no unit, a unit past the last row
    2 * ROUND,        # two full rounds: first and last, no steady one
    3 * ROUND + 1,    # 3,841: three rounds and a row
])
@pytest.mark.parametrize("L,N", [(768, 1), (768, 2), (1024, 1), (1024, 2)])
def test_helper_form_same_bits_as_parent_and_20_step_launches(models, L, N, B):
    st, mh, m4 = models(L, N)
    check_launch(st, mh, m4, B)


def test_helper_form_fifteen_rounds(models):
    """19,213 rows (the benchmark's dump size): 15 rounds and a ragged sixteenth."""
    st, mh, m4 = models(1024, 2)
    B = 19213
    idx = np.unique(np.r_[0:64, np.random.default_rng(7).choice(B, 512, replace=False), B - 96:B])
    check_launch(st, mh, m4, B, idx)


def test_helper_form_integer_model_bit_exact():
    """tests/exact_models.py: every partial sum an integer below 2^23, so the launch equals the
    oracle's float32 forward bit for bit whatever its tiling -- a wrong slice, a stale hand-off or a
    partial read before it was written changes an integer."""
    B = 33 * 64 + 1
    for L, N in ((1024, 2), (768, 1)):
        cfg, st = exact_models.integer_state(L, N, nnz=8)
        x = exact_models.integer_inputs(B, seed=B + L)
        ref = exact_models.exact_forward(st, x)
        m = model(cfg, st)
        y = m.serve_device(torch.from_numpy(x).cuda())
        assert kname(m) == HELPERS, kname(m)
        torch.cuda.synchronize()
        m.serve_check()
        assert np.array_equal(y.cpu().numpy(), ref), (L, N)
        m.close()


def test_state_carried_between_launches(models):
    """The flag banks and epoch words across launches: three helper-form launches back to back, then a
    20-step launch between two long ones -- every launch equal to its first."""
    st, mh, _ = models(1024, 2)
    rng = np.random.default_rng(23)
    xl = torch.from_numpy(rng.standard_normal((2 * ROUND + 80 + 3, 32)).astype(np.float32)).cuda()
    xs = torch.from_numpy(rng.standard_normal((ROUND, 32)).astype(np.float32)).cuda()
    yl0 = mh.serve_device(xl)
    assert kname(mh) == HELPERS
    for _ in range(2):
        yl = mh.serve_device(xl)
        torch.cuda.synchronize()
        assert torch.equal(yl, yl0)
    ys0 = mh.serve_device(xs)
    assert kname(mh) == SHORT
    for _ in range(2):
        yl = mh.serve_device(xl)
        assert kname(mh) == HELPERS
        ys = mh.serve_device(xs)
        assert kname(mh) == SHORT
        yl2 = mh.serve_device(xl)
        torch.cuda.synchronize()
        assert torch.equal(yl, yl0) and torch.equal(ys, ys0) and torch.equal(yl2, yl0)
    mh.serve_check()
    ro, _ = ref_mlp.forward(st, xl.cpu().numpy()[-200:], False, 1.0, 0, 0, 0)
    close(yl0.cpu().numpy()[-200:], ro)


def test_late_xcd(monkeypatch, models):
    """Test hook P3D_SERVE_TEST_DELAY: every workgroup of XCD 3 starts ~1 ms late on every other call;
    each launch has the bits of the undelayed model."""
    st, ref, _ = models(1024, 2)
    cfg = ref_mlp.Cfg(linear_size=1024, num_layers=2, residual=True, batch_norm=True)
    monkeypatch.setenv("P3D_SERVE_TEST_DELAY", "300,3")
    m = model(cfg, st)
    monkeypatch.delenv("P3D_SERVE_TEST_DELAY")
    rng = np.random.default_rng(43)
    for call in range(2):
        x = torch.from_numpy(rng.standard_normal((3 * ROUND, 32)).astype(np.float32)).cuda()
        y = m.serve_device(x)
        assert kname(m) == HELPERS
        y0 = ref.serve_device(x)
        torch.cuda.synchronize()
        m.serve_check()
        assert torch.equal(y, y0), "launch %d (delayed=%s) differs" % (call, call % 2 == 0)
    m.close()


def test_nan_row_in_the_second_round(models):
    """One NaN input row in the middle of round 2: that output row is NaN, every other row keeps its
    bits, no error is flagged (no wait of either role depends on a floating-point value)."""
    st, mh, _ = models(1024, 2)
    B, bad = 2 * ROUND, ROUND + ROUND // 2
    x = np.random.default_rng(5).standard_normal((B, 32)).astype(np.float32)
    y0 = mh.serve_device(torch.from_numpy(x).cuda())
    x[bad, 7] = np.nan
    y = mh.serve_device(torch.from_numpy(x).cuda())
    assert kname(mh) == HELPERS
    torch.cuda.synchronize()
    mh.serve_check()
    f = _p3d.ctypes.c_int32(-1)
    _p3d.check(_p3d.lib().p3d_error_flags(mh._h, _p3d.ctypes.byref(f), 0), "p3d_error_flags")
    assert f.value == 0, f.value
    assert bool(torch.isnan(y[bad]).all())
    keep = torch.ones(B, dtype=torch.bool, device="cuda")
    keep[bad] = False
    assert torch.equal(y[keep], y0[keep])
