"""Inputs with non-finite rows and their finite twins, shared by tests/test_nonfinite_oracle.py (the
references alone) and tests/test_gpu_nonfinite.py (the HIP kernels against them).

The rule under test ("Non-finite input"): a row that holds a NaN or an Inf leaves every
forward as a NaN row, makes the loss NaN and every gradient NaN -- as np.maximum and the mask
products of the oracles do -- and changes no other row by a single bit.

A *twin* is the same array with each bad row holding finite values from the same generator: the
twin is drawn first and the poison written over a copy of it, so bad and twin agree bit for bit in
every good row.
"""
import numpy as np

KINDS = ("nan_first", "nan_last", "pos_inf", "neg_inf", "nan_row")


def poison_row(row, kind):
    """Write the poison of `kind` into one row (in place): a NaN in column 0, a NaN in the last
    column (next to the K padding of the contraction), a +Inf, a -Inf, or NaN in every column."""
    n = row.shape[0]
    if kind == "nan_first":
        row[0] = np.nan
    elif kind == "nan_last":
        row[n - 1] = np.nan
    elif kind == "pos_inf":
        row[n // 3] = np.inf
    elif kind == "neg_inf":
        row[n - 2] = -np.inf
    elif kind == "nan_row":
        row[:] = np.nan
    else:
        raise ValueError(kind)


def edge_rows(B, extra=()):
    """The rows at the edges of the row tiles: 0 and B - 1 (a ragged last row, which padding
    repeats), 15 / 16 (the MFMA row tile), 63 / 64 (a batch-64 step), 79 / 80 and 159 / 160 (the
    80-row units of the pair form), where B allows; plus `extra`."""
    rows = {0, B - 1}
    for r in (15, 16, 63, 64, 79, 80, 159, 160) + tuple(extra):
        if 0 < r < B - 1:
            rows.add(r)
    return sorted(rows)


def poisoned(shape, rows, seed, kinds=KINDS, scale=1.0):
    """(bad, twin, mask): float32 arrays of `shape`, the poison kinds dealt over `rows` in turn (so
    every kind appears once five rows are bad), mask[r] = row r is bad."""
    rng = np.random.default_rng(seed)
    twin = (scale * rng.standard_normal(shape)).astype(np.float32)
    bad = twin.copy()
    mask = np.zeros(shape[0], bool)
    for i, r in enumerate(rows):
        poison_row(bad[r], kinds[i % len(kinds)])
        mask[r] = True
    return bad, twin, mask


def check_rows(got_bad, got_twin, mask, what=""):
    """Assertions 1 and 2 of the rule on one output array [B, ...]: the bad rows are NaN in every
    column, every other row has the bits of the twin's run."""
    got_bad, got_twin = np.asarray(got_bad), np.asarray(got_twin)
    assert got_bad.shape == got_twin.shape and got_bad.shape[0] == mask.shape[0], what
    nan = np.isnan(got_bad).reshape(len(mask), -1)
    short = [int(r) for r in np.nonzero(mask)[0] if not nan[r].all()]
    assert not short, "%s: bad rows with non-NaN columns: %s (%d of %d columns NaN in row %d)" % (
        what, short[:8], int(nan[short[0]].sum()), nan.shape[1], short[0])
    assert not np.isnan(got_twin).any(), "%s: the twin's run holds NaN" % what
    np.testing.assert_array_equal(got_bad[~mask], got_twin[~mask], err_msg="%s: good rows differ from the twin's" % what)


def all_nan(a):
    a = np.asarray(a)
    return bool(a.size) and bool(np.isnan(a).all())


# ---- the lifter's forward cases: name -> (L, N, residual, batch_norm, max_norm, predict_14, B, bad rows,
# kinds).  Bad rows: a list is taken as it is; None is edge_rows(B); a tuple adds its rows to edge_rows(B).
# One table for the host test of the oracle and the GPU test of the forms.
_T, _F = True, False
LIFTER_CASES = {
    # batch <= 4 (k_gemv forms): B 1 -- the whole output NaN -- and B 4 with row 2 bad
    "L64_B1": (64, 2, _T, _T, _F, _F, 1, [0], ("nan_last",)),
    "L64_B4": (64, 2, _T, _T, _F, _F, 4, [2], ("pos_inf",)),
    "L1024_B1": (1024, 2, _T, _T, _F, _F, 1, [0], ("nan_row",)),
    "L1024_B4": (1024, 2, _T, _T, _F, _F, 4, [2], ("neg_inf",)),
    # the batch-64 layer kernels: a ragged row tile (37) and 13 row tiles (200)
    "bn_B37": (256, 2, _T, _T, _F, _F, 37, (31,), KINDS),
    "bn_B200": (256, 2, _T, _T, _F, _F, 200, None, KINDS),
    "nobn_B37": (256, 2, _T, _F, _F, _F, 37, (31,), KINDS),
    "nobn_B200": (256, 2, _T, _F, _F, _F, 200, None, KINDS),
    "maxnorm_B37": (256, 2, _T, _T, _T, _F, 37, (31,), KINDS),
    "maxnorm_B200": (256, 2, _T, _T, _T, _F, 200, None, KINDS),
    "p14_B37": (256, 2, _T, _T, _F, _T, 37, (31,), KINDS),
    "p14_B200": (256, 2, _T, _T, _F, _T, 200, None, KINDS),
    # k_gemm_f32 (M >= 256): 128-row tiles
    "gemm_B300": (1024, 2, _T, _T, _F, _F, 300, (127, 128, 255, 256), KINDS),
    # p3d_serve
    "serve_L256_B327": (256, 1, _T, _T, _F, _F, 327, (319, 320), KINDS),
    "serve_L384_B327": (384, 1, _T, _T, _F, _F, 327, (319, 320), KINDS),
    "serve_L1024_B327": (1024, 2, _T, _T, _F, _F, 327, (319, 320), KINDS),
    "serve_L1024_B1280": (1024, 2, _T, _T, _F, _F, 1280, (639, 640, 1199, 1200), KINDS),
    # 33 steps: a first round of 1,280 rows, a last round of 832 = ten 80-row units and a 32-row tail
    "rounds_B2112": (1024, 2, _T, _T, _F, _F, 2112, (1279, 1280, 1295, 1296, 1359, 1360, 2079, 2080), KINDS),
    "L1024_B37": (1024, 2, _T, _T, _F, _F, 37, (31,), KINDS),
    # bf16 path (vs ref_mlp.forward_bf16)
    "bf16_B200": (512, 1, _T, _T, _F, _F, 200, None, KINDS),
}
_lifter = {}


def lifter_case(name):
    """The inputs of LIFTER_CASES[name] and the float64 oracle's eval forward of both (bf16_*: the
    emulated-bf16 oracle), computed once: dict(cfg, st, bad, twin, mask, ref_bad, ref_twin)."""
    if name not in _lifter:
        from oracle import ref_mlp
        L, N, res, bn, mx, p14, B, rows, kinds = LIFTER_CASES[name]
        cfg = ref_mlp.Cfg(linear_size=L, num_layers=N, residual=res, batch_norm=bn, max_norm=mx, predict_14=p14)
        st = ref_mlp.init_state(cfg, seed=1, bn_seed=2)
        if rows is None or isinstance(rows, tuple):
            rows = edge_rows(B, rows or ())
        bad, twin, mask = poisoned((B, 32), rows, seed=1000 + B, kinds=kinds)
        with np.errstate(invalid="ignore", over="ignore"):
            if name.startswith("bf16"):
                ref_bad, ref_twin = ref_mlp.forward_bf16(st, bad), ref_mlp.forward_bf16(st, twin)
            else:
                ref_bad, ref_twin = ref_mlp.forward(st, bad, False)[0], ref_mlp.forward(st, twin, False)[0]
        for a in (bad, twin, mask, ref_bad, ref_twin):
            a.setflags(write=False)
        _lifter[name] = dict(cfg=cfg, st=st, B=B, bad=bad, twin=twin, mask=mask, ref_bad=ref_bad, ref_twin=ref_twin)
    return _lifter[name]


def seq_case(shape, lens, bad, seed):
    """A concatenated sequence batch for vae_seq_oracle.filter: predictions, eps, targets, offsets,
    and the poisoned predictions.  `bad` maps a sequence index to the frame k that takes a NaN (in
    one column): by the recurrence every frame >= k of that sequence is NaN, nothing else.
    Returns a dict with pred_bad, pred (the twin), eps, tgt, off and the frame mask."""
    out, lat = shape[4], shape[2]
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(off[-1])
    pred = rng.standard_normal((N, out)).astype(np.float32)
    eps = rng.standard_normal((N, lat)).astype(np.float32)
    tgt = rng.standard_normal((N, out)).astype(np.float32)
    pred_bad = pred.copy()
    mask = np.zeros(N, bool)
    for i, (s, k) in enumerate(sorted(bad.items())):
        assert 0 <= k < lens[s]
        pred_bad[off[s] + k, (7 * i + 5) % out] = np.nan
        mask[off[s] + k:off[s + 1]] = True
    seq_mask = np.zeros(len(lens), bool)
    seq_mask[list(bad)] = True
    return dict(pred_bad=pred_bad, pred=pred, eps=eps, tgt=tgt, off=off, mask=mask, seq_mask=seq_mask, N=N)


def clip_case(n, seed, frame, col):
    """Raw OpenPose rows [n, 36] in the usual range, no dropped joints, and the same rows with one
    NaN keypoint coordinate at (frame, col).  With smoothing the median windows spread it over the
    frames whose window holds `frame`; the mask names them (window_frames)."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(100.0, 900.0, (n, 36))
    xy[:, 2:4] = rng.uniform(540.0, 700.0, (n, 2))
    bad = xy.copy()
    bad[frame, col] = np.nan
    return bad, xy


def window_frames(n, frame, smooth):
    """The frames whose median window (clip_oracle.smooth) contains `frame`."""
    mask = np.zeros(n, bool)
    if not smooth or n == 1:
        mask[frame] = True
        return mask
    for i in range(n):
        if i < 4:
            rows = range(i, i + 4)
        elif i >= n - 4:
            rows = range(i - 3, i + 1)
        else:
            rows = range(i - 3, i + 4)
        mask[i] = frame in rows
    return mask


# ---- the VAE filter's cases (tests/vae_oracle.py shapes) ------------------------------------------
VAE_SHAPES = {
    "default": (48, (40, 32), 24, (32, 40), 48),
    "edge264": (264, (8,), 8, (24,), 48),
    "wide": (1360, (40, 32), 24, (32, 40), 48),
    "edge96": (96, (8,), 8, (24,), 48),
}
VAE_FACTORS = (100.0, 0.02, 1.0)
# 20 sequences: a full 16-sequence tile and a second one of four; the poisoned sequences sit at tile
# positions 5 (first tile), 0 and 3 (second tile), poisoned at a middle, the first and the last frame
SEQ_LENS = [5, 3, 7, 4, 6, 9, 2, 8, 5, 4, 3, 6, 7, 5, 4, 8, 6, 3, 5, 4]
SEQ_BAD = {5: 2, 16: 0, 19: 3}


def vae_params(shape, seed):
    """Glorot kernels and small random biases (as the VAE GPU tests' rand_params)."""
    import vae_oracle as vo
    P = vo.init_params(shape, seed)
    rng = np.random.default_rng(seed + 1)
    for k in P:
        if k.endswith("/bias"):
            P[k] = (0.1 * rng.standard_normal(P[k].shape)).astype(np.float32)
    return P


def vae_case(name, B, rows, seed, kinds=("nan_first",)):
    """x (bad and twin), t, eps for a VAE shape."""
    shape = VAE_SHAPES[name]
    bad, twin, mask = poisoned((B, shape[0]), rows, seed, kinds)
    rng = np.random.default_rng(seed + 1000)
    t = rng.standard_normal((B, shape[4])).astype(np.float32)
    eps = rng.standard_normal((B, shape[2])).astype(np.float32)
    return dict(shape=shape, x_bad=bad, x=twin, mask=mask, t=t, eps=eps)
