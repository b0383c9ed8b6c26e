"""k_serve6_rounds: launches of more than 32 batch-64 steps on the pair form, rounds run back to back.

A round is 1,280 rows on 256 CUs (8 XCDs x two 80-row units).  The long launch keeps only its
first round's prologue and its last round's closing output phase; in between the next round's
input layers are computed at the boundaries of the last two blocks and a round's output layer
runs at a block boundary of the next round (csrc/p3d_serve6.h).  Every output tile keeps its
association, so a long launch must have the BITS of the same rows served 1,280 at a time by the
unchanged one-round kernel k_serve6<4, 3, 2, 5, true>, and the oracle's values within the
tolerance tests/test_gpu_serve.py uses for k_serve6 launches (5e-5 abs and rel).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import _p3d  # noqa: E402
import linear_model  # noqa: E402
from oracle import ref_mlp  # noqa: E402

ROUND = 1280
ROUNDS = "k_serve6_rounds<4, 3, 2, 5>"
SHORT = "k_serve6<4, 3, 2, 5, true>"


def make(cfg, seed=1, bn_seed=2):
    st = ref_mlp.init_state(cfg, seed=seed, bn_seed=bn_seed)
    m = linear_model.LinearModel(cfg.linear_size, cfg.num_layers, cfg.residual, cfg.batch_norm, cfg.max_norm,
                                 64, 1e-3, "/tmp/p3d_test", cfg.predict_14, seed=11, max_batch=64)
    m.set_weights({**st.params, **st.moving})
    return st, m


def close(a, b, atol=5e-5, rtol=5e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b)
    tol = atol + rtol * np.abs(b)
    assert np.all(err <= tol), "max err %.3g (at ref %.3g)" % (err.max(), b.flat[np.argmax(err - tol)])


def kname(m):
    name = _p3d.ctypes.create_string_buffer(128)
    _p3d.check(_p3d.lib().p3d_kernel_name(m._h, 3, name, 128), "p3d_kernel_name")
    return name.value.decode()


def chunked(m, xd, check_name=True):
    """The rows of xd served one round (1,280 rows) per launch: the unchanged one-round kernel."""
    out = []
    for i in range(0, xd.shape[0], ROUND):
        out.append(m.serve_device(xd[i:i + ROUND]))
        if check_name and xd.shape[0] - i >= ROUND:
            assert kname(m) == SHORT, kname(m)
    return torch.cat(out)


def oracle_rows(B, seed):
    """All rows of a small launch; else the first 64, a seeded sample of 512 and the tail."""
    if B <= 2 * ROUND:
        return np.arange(B)
    return np.unique(np.r_[0:64, np.random.default_rng(seed).choice(B, 512, replace=False), B - 96:B])


CFG2 = ref_mlp.Cfg(linear_size=1024, num_layers=2, residual=True, batch_norm=True)


@pytest.fixture(scope="module")
def cfg2_model():
    st, m = make(CFG2)
    yield st, m
    m.close()


@pytest.mark.parametrize("B", [
    2 * ROUND,                # two exact rounds: first + last, no steady round
    3 * ROUND,                # one steady round
    ROUND + 1,                # second round: one unit on one group, its partner past the last row, 7 groups idle
    3 * ROUND + 9 * 80 + 7,   # odd unit count: some groups a pair, one a lone unit, a ragged tail
    33 * 64,                  # the first size that takes the new form
])
def test_rounds_same_bits_as_one_round_launches(monkeypatch, cfg2_model, B):
    """(1,281 rows are 21 steps, which the default choice does not count as a long launch: that case
    runs on a model made with P3D_SERVE6_MAX_NB=20, so the launch takes the new form and its 1,280-row
    chunk the one-round kernel, as everywhere else.)"""
    st, m = cfg2_model
    if B <= 32 * 64:
        monkeypatch.setenv("P3D_SERVE6_MAX_NB", "20")
        _, m = make(CFG2)
        monkeypatch.delenv("P3D_SERVE6_MAX_NB")
    x = np.random.default_rng(B).standard_normal((B, 32)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    y = m.serve_device(xd)
    assert kname(m) == ROUNDS, kname(m)
    yc = chunked(m, xd)
    torch.cuda.synchronize()
    m.serve_check()
    assert not bool(torch.isnan(y).any())
    assert torch.equal(y, yc), "rows differ: %d" % int((y != yc).any(dim=1).sum())
    idx = oracle_rows(B, B)
    ro, _ = ref_mlp.forward(st, x[idx], False, 1.0, 0, 0, 0)
    close(y.cpu().numpy()[idx], ro)
    if m is not cfg2_model[1]:
        m.close()


@pytest.mark.parametrize("L,N,residual,batch_norm,max_norm,p14", [
    (768, 1, True, True, False, False),      # the narrowest width: 12 k-groups per wave, members with one tile
    (1024, 3, True, True, True, False),      # three blocks (the rotation wraps differently), max-norm
    (1024, 2, False, False, False, False),   # no BN, no residual
    (1024, 2, True, True, False, True),      # --predict_14: 42 outputs
])
def test_rounds_variants_vs_oracle_and_one_round_launches(L, N, residual, batch_norm, max_norm, p14):
    """Three rounds and a tail of 85 rows (two units on one group)."""
    cfg = ref_mlp.Cfg(linear_size=L, num_layers=N, residual=residual, batch_norm=batch_norm, max_norm=max_norm,
                      predict_14=p14)
    st, m = make(cfg)
    B = 3 * ROUND + 85
    x = np.random.default_rng(L + N).standard_normal((B, 32)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    y = m.serve_device(xd)
    assert kname(m) == ROUNDS, kname(m)
    yc = chunked(m, xd, check_name=(L == 1024))
    torch.cuda.synchronize()
    m.serve_check()
    assert torch.equal(y, yc), "rows differ: %d" % int((y != yc).any(dim=1).sum())
    idx = oracle_rows(B, L)
    ro, _ = ref_mlp.forward(st, x[idx], False, 1.0, 0, 0, 0)
    assert y.shape[1] == ro.shape[1]
    close(y.cpu().numpy()[idx], ro)
    m.close()


@pytest.mark.parametrize("L,env", [(256, None), (2048, None), (1024, "0")])
def test_long_launches_the_pair_form_does_not_cover_stay_on_serve5(monkeypatch, L, env):
    """Widths outside 768..1024 and P3D_SERVE6=0 keep k_serve5 for a 40-step launch."""
    cfg = ref_mlp.Cfg(linear_size=L, num_layers=1 if L != 1024 else 2, residual=True, batch_norm=True)
    if env is not None:
        monkeypatch.setenv("P3D_SERVE6", env)
    st, m = make(cfg)
    monkeypatch.delenv("P3D_SERVE6", raising=False)
    B = 64 * 40
    x = np.random.default_rng(L).standard_normal((B, 32)).astype(np.float32)
    y = m.serve_device(torch.from_numpy(x).cuda())
    assert kname(m).startswith("k_serve5<"), kname(m)
    torch.cuda.synchronize()
    m.serve_check()
    idx = oracle_rows(B, L)
    ro, _ = ref_mlp.forward(st, x[idx], False, 1.0, 0, 0, 0)
    close(y.cpu().numpy()[idx], ro)
    m.close()


def test_rounds_graph_replay_follows_inputs_and_parameters():
    """A 3-round launch captured in a HIP graph, replayed 5 times with new inputs and once with new
    parameters in between: every replay equals an eager call (the banks alternate on the device, the
    epilogue constants are re-formed inside the graph)."""
    st, m = make(CFG2)
    B = 3 * ROUND
    x = torch.zeros((B, 32), device="cuda")
    y = torch.zeros((B, 48), device="cuda")
    m.serve_device(x, out=y)                          # warm-up (tables, buffers)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        m.serve_device(x, out=y)
    assert kname(m) == ROUNDS, kname(m)
    rng = np.random.default_rng(22)
    for rep in range(5):
        x.copy_(torch.from_numpy(rng.standard_normal((B, 32)).astype(np.float32)))
        if rep == 3:
            st = ref_mlp.init_state(CFG2, seed=31, bn_seed=32)
            m.set_weights({**st.params, **st.moving})
        g.replay()
        torch.cuda.synchronize()
        ye = m.serve_device(x)
        torch.cuda.synchronize()
        assert torch.equal(y, ye), rep
    m.serve_check()
    idx = oracle_rows(B, 5)
    ro, _ = ref_mlp.forward(st, x.cpu().numpy()[idx], False, 1.0, 0, 0, 0)
    close(y.cpu().numpy()[idx], ro)
    del g
    m.close()


def test_rounds_and_one_round_launches_alternate_on_one_model(cfg2_model):
    """The epoch / bank words survive a launch whose groups ran different round counts (2 rounds and
    a tail on one group): long and 20-step launches alternate 6 times, bits unchanged."""
    st, m = cfg2_model
    rng = np.random.default_rng(23)
    xl = torch.from_numpy(rng.standard_normal((2 * ROUND + 80 + 3, 32)).astype(np.float32)).cuda()
    xs = torch.from_numpy(rng.standard_normal((ROUND, 32)).astype(np.float32)).cuda()
    yl0, ys0 = m.serve_device(xl), m.serve_device(xs)
    for _ in range(6):
        yl = m.serve_device(xl)
        assert kname(m) == ROUNDS
        ys = m.serve_device(xs)
        assert kname(m) == SHORT
        torch.cuda.synchronize()
        assert torch.equal(yl, yl0) and torch.equal(ys, ys0)
    m.serve_check()
    ro, _ = ref_mlp.forward(st, xl.cpu().numpy()[-200:], False, 1.0, 0, 0, 0)
    close(yl0.cpu().numpy()[-200:], ro)


def test_rounds_late_xcd_group(monkeypatch, cfg2_model):
    """Test hook P3D_SERVE_TEST_DELAY: every workgroup of XCD 3 starts ~1 ms late on every other call
    of a 3-round launch; every launch has the bits of the undelayed model."""
    st, ref = cfg2_model
    monkeypatch.setenv("P3D_SERVE_TEST_DELAY", "300,3")
    _, m = make(CFG2)
    monkeypatch.delenv("P3D_SERVE_TEST_DELAY")
    rng = np.random.default_rng(43)
    for call in range(4):
        x = torch.from_numpy(rng.standard_normal((3 * ROUND, 32)).astype(np.float32)).cuda()
        y = m.serve_device(x)
        assert kname(m) == ROUNDS
        y0 = ref.serve_device(x)
        torch.cuda.synchronize()
        m.serve_check()
        assert torch.equal(y, y0), "launch %d (delayed=%s) differs" % (call, call % 2 == 0)
    m.close()


def test_rounds_failed_launch_reports_and_fills_nan(monkeypatch, cfg2_model):
    """Test hook P3D_SERVE_TEST_FAULT (a placement the launch cannot use) on a 3-round launch: every
    row NaN, further launches refused until serve_check reports it (once).  The hook stays with its
    model, so the clean launch after the check is a healthy model's on the same device."""
    st, ref = cfg2_model
    monkeypatch.setenv("P3D_SERVE_TEST_FAULT", "1")
    _, m = make(CFG2)
    monkeypatch.delenv("P3D_SERVE_TEST_FAULT")
    x = torch.randn((3 * ROUND, 32), device="cuda", generator=torch.Generator("cuda").manual_seed(6))
    y = torch.zeros((x.shape[0], 48), device="cuda")
    m.serve_device(x, out=y)
    assert kname(m) == ROUNDS
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()), "failed launch left non-NaN rows"
    with pytest.raises(_p3d.P3DError, match="earlier launch failed"):
        m.serve_device(x, out=y)
    with pytest.raises(_p3d.P3DError, match="synchronisation timed out"):
        m.serve_check()
    m.serve_check()                                   # reported once
    m.close()
    y0 = ref.serve_device(x)
    assert kname(ref) == ROUNDS
    torch.cuda.synchronize()
    ref.serve_check()
    assert torch.equal(y0, chunked(ref, x))
    idx = oracle_rows(x.shape[0], 6)
    ro, _ = ref_mlp.forward(st, x.cpu().numpy()[idx], False, 1.0, 0, 0, 0)
    close(y0.cpu().numpy()[idx], ro)
