"""numpy restatement of the temporal filter's recurrence (src/3d_pose_vae_filter_kin.py:323-342,
evaluate()) over tests/vae_oracle.forward, in float64 or float32, batched over sequences -- what
csrc/p3d_vae_seq.h is tested against.

For one sequence with lifter predictions p_0 .. p_{T-1}, eps rows e_0 .. e_{T-1} and
seq_len = in / out:

    buffer = [p_0] * seq_len
    for f in range(T):
        buffer = buffer[1:] + [p_f]
        r_f = VAE(concat(buffer), eps=e_f)      # models.py:79-80 draws eps also with training=False
        buffer[-1] = r_f
        err_pred[f] = mean((y_f - p_f)^2);  err_ref[f] = mean((y_f - r_f)^2)     # losses.py:53-56

`filter` runs every sequence of a concatenated [N, out] array at once (one VAE forward per frame
index over the sequences still running) and carries the buffer's first seq_len - 1 groups in
`state` / `started` so that a stream can be filtered in chunks; `filter_literal` is the loop above,
word for word, with a Python list.
"""
import numpy as np

import vae_oracle as vo


def seq_len_of(shape):
    assert shape[0] % shape[4] == 0
    return shape[0] // shape[4]


def new_state(shape, S, dt=np.float64):
    return np.zeros((S, (seq_len_of(shape) - 1) * shape[4]), dt), np.zeros(S, np.int32)


def filter(P, shape, pred, seq_off, eps, target=None, state=None, dt=np.float64, check=None):
    """Returns {ref [N, out], frame_err [N, 2], seq_err [S, 2]} (the errors only with a target).
    `state` = (state, started) is updated in place.  `check(f, rows, x, cache)` is called per frame
    index with the windows and the forward's cache (for the exactness proofs)."""
    out, L = shape[4], seq_len_of(shape)
    seq_off = np.asarray(seq_off, np.int64)
    S, N = len(seq_off) - 1, len(pred)
    assert seq_off[0] == 0 and seq_off[-1] == N and (np.diff(seq_off) >= 0).all()
    lens = np.diff(seq_off)
    pred = pred.astype(dt)
    ref = np.zeros((N, out), dt)
    ferr = np.zeros((N, 2), dt)
    serr = np.zeros((S, 2), np.float64)
    buf = np.zeros((S, L * out), dt)
    for s in np.nonzero(lens > 0)[0]:
        p0 = pred[seq_off[s]]
        if state is not None and state[1][s]:
            buf[s, out:] = state[0][s]             # (the first frame's shift moves them to the front)
        else:
            buf[s] = np.tile(p0, L)
    for f in range(int(lens.max()) if S else 0):
        rows = np.nonzero(lens > f)[0]
        g = seq_off[rows] + f
        buf[rows] = np.concatenate([buf[rows, out:], pred[g]], axis=1)
        c = vo.forward(P, shape, buf[rows], eps[g], dt)
        if check is not None:
            check(f, rows, buf[rows], c)
        r = c["y"]
        buf[rows, (L - 1) * out:] = r
        ref[g] = r
        if target is not None:
            t = target[g].astype(dt)
            ferr[g, 0] = np.mean(np.square(t - pred[g]), axis=-1, dtype=dt)
            ferr[g, 1] = np.mean(np.square(t - r), axis=-1, dtype=dt)
            serr[rows] += ferr[g].astype(np.float64)
    if state is not None:
        run = lens > 0
        # what the next chunk's first shift keeps: the last seq_len - 1 groups
        state[0][run] = buf[run, out:]
        state[1][run] = 1
    res = {"ref": ref}
    if target is not None:
        res["frame_err"], res["seq_err"] = ferr, serr
    return res


def filter_literal(P, shape, pred, seq_off, eps, target=None, dt=np.float64):
    """The reference's loop per sequence and frame with a Python list buffer."""
    out, L = shape[4], seq_len_of(shape)
    N, S = len(pred), len(seq_off) - 1
    ref, ferr, serr = np.zeros((N, out), dt), np.zeros((N, 2), dt), np.zeros((S, 2), np.float64)
    for s in range(S):
        a, b = int(seq_off[s]), int(seq_off[s + 1])
        buffer = []
        for g in range(a, b):
            p = pred[g].astype(dt)
            if g == a:
                buffer = [p for _ in range(L)]
            buffer.append(p)
            buffer.pop(0)
            r = vo.forward(P, shape, np.concatenate(buffer)[None, :], eps[g:g + 1], dt)["y"][0]
            buffer[-1] = r
            ref[g] = r
            if target is not None:
                t = target[g].astype(dt)
                ferr[g] = (np.mean(np.square(t - p), dtype=dt), np.mean(np.square(t - r), dtype=dt))
                serr[s] += ferr[g].astype(np.float64)
    res = {"ref": ref}
    if target is not None:
        res["frame_err"], res["seq_err"] = ferr, serr
    return res


def split(seq_off, at):
    """The two chunks of every sequence cut `at` frames in (or at its end when shorter): returns
    (frame indices of chunk 1, its offsets, frame indices of chunk 2, its offsets)."""
    seq_off = np.asarray(seq_off, np.int64)
    lens = np.diff(seq_off)
    n1 = np.minimum(lens, at)
    i1 = np.concatenate([np.arange(o, o + n) for o, n in zip(seq_off[:-1], n1)] + [np.zeros(0, np.int64)])
    i2 = np.concatenate([np.arange(o + n, e) for o, n, e in zip(seq_off[:-1], n1, seq_off[1:])] + [np.zeros(0, np.int64)])
    o1 = np.concatenate([[0], np.cumsum(n1)])
    o2 = np.concatenate([[0], np.cumsum(lens - n1)])
    return i1.astype(np.int64), o1.astype(np.int64), i2.astype(np.int64), o2.astype(np.int64)


_exact = {}


def exact_case():
    """The proven integer case of the in144 filter: vae_exact.integer_params, predictions integer in
    [-2, 2], eps even integers in {-2, 0, 2}, 20 sequences of 12 frames.  Per frame the float32 and
    float64 oracles agree bit for bit, every value is an integer and every contraction's sum of
    absolute values stays below 2^23 -- so any summation order gives these bits."""
    if "k" in _exact:
        return _exact["k"]
    import vae_exact as ve
    shape = (144, (40, 32), 24, (32, 40), 48)
    P = ve.integer_params(shape)
    rng = np.random.default_rng(77)
    S, T = 20, 12
    pred = rng.integers(-2, 3, size=(S * T, 48)).astype(np.float32)
    eps = (2 * rng.integers(-1, 2, size=(S * T, 24))).astype(np.float32)
    seq_off = np.arange(S + 1, dtype=np.int64) * T
    a = {k: np.abs(v.astype(np.float64)) for k, v in P.items()}
    caches = {}

    def check64(f, rows, x, c):
        caches[f] = (x.copy(), {k: c[k].copy() for k in ("y", "mean", "log_var", "z")})
        # absolute contraction sums of every dense layer of this frame
        acts = list(c["enc_in"]) + [c["h"], c["h"]] + list(c["dec_in"]) + [c["d"]]
        for (name, K, N), ain in zip(vo.layer_names(shape), acts):
            worst = float((np.abs(ain) @ a[name + "/kernel"] + a[name + "/bias"]).max())
            assert worst < 2.0 ** 23, (f, name, worst)

    def check32(f, rows, x, c):
        x64, c64 = caches[f]
        assert x.dtype == np.float32 and np.array_equal(x, x64)
        for k in ("y", "mean", "log_var", "z"):
            assert c[k].dtype == np.float32 and np.array_equal(c[k], c64[k]), (f, k)
            assert np.array_equal(c[k], np.round(c[k])), (f, k)
        assert not c["log_var"].any()

    r64 = filter(P, shape, pred, seq_off, eps, dt=np.float64, check=check64)
    r32 = filter(P, shape, pred, seq_off, eps, dt=np.float32, check=check32)
    assert r32["ref"].dtype == np.float32 and np.array_equal(r32["ref"], r64["ref"])
    assert len(caches) == T
    k = {"P": P, "shape": shape, "pred": pred, "eps": eps, "seq_off": seq_off, "ref": r32["ref"],
         "max_abs": float(np.abs(r64["ref"]).max())}
    for v in (pred, eps, seq_off, r32["ref"]):
        v.setflags(write=False)
    _exact["k"] = k
    return k
