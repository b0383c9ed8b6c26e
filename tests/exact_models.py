"""Integer-valued models: parity checks that need no tolerance (round 6).

Every weight is 0 or +-1 (a few non-zeros per column), every bias, BN shift and moving mean a small
integer, BN gamma 1 or 2, the moving variance 0.999f -- so that in float32 var + eps == 1.0
exactly and the eval-BN scale gamma / sqrt(var + eps) is gamma itself -- and the inputs integers in
[-4, 4].  Then every product, partial sum, BN affine, ReLU and residual add of the forward is an
integer below 2^24, which float32 represents exactly whatever the summation order: the GPU paths
(any tiling, K split, wave association, launch shape) and the oracle's float32 forward
(oracle/ref_mlp.forward, dt=float32) must agree BIT FOR BIT, at the BASELINE configurations' full
sizes.  A wrong k-slice, a skipped or doubled tile, a stale hand-off or a misplaced row changes an
integer and fails.  bf16 paths: +-1 weights and small integers are exact in bf16, every activation
is rounded to bf16 (round-to-nearest-even of an exactly accumulated integer) by the kernels and by
the oracle's bf16 emulation alike, so they too must agree bit for bit.

Training: on a model without BN the training forward and the backward add only dropout (at keep 0.5
an exact x2 under a mask from the Philox stream the kernels share with the oracle) and the
contractions x^T dz, dz W^T and sum dz; with an integer dy in [-2, 2] every gradient is an integer
too, and exact_backward proves, per case, that no partial sum of any contraction can leave the
exact range -- so p3d_backward's gradients must equal the oracle's bit for bit through every launch
form.  BN-train (1 / sqrt(var + eps)), max-norm (a Frobenius norm), Adam and the fused MSE's dy
(a 1 / (B D) factor) are not exact and stay with the tolerance tests.

(The test data is synthetic; the arithmetic it checks is that of src/linear_model.py:92-128 with
BN in inference mode -- the reference's own outputs for it are not available here)"""
import numpy as np

from oracle import ref_mlp


def integer_state(L, N, nnz=8, seed=5, residual=True, batch_norm=True, predict_14=False):
    cfg = ref_mlp.Cfg(linear_size=L, num_layers=N, residual=residual, batch_norm=batch_norm,
                      predict_14=predict_14)
    st = ref_mlp.init_state(cfg, seed=1, bn_seed=2)
    rng = np.random.default_rng(seed)
    for name, v in list(st.params.items()):
        leaf = name.split("/")[-1]
        if leaf.startswith("w"):
            K, Nn = v.shape
            w = np.zeros((K, Nn), np.float32)
            for j in range(Nn):
                rows = rng.choice(K, size=min(nnz, K), replace=False)
                w[rows, j] = rng.choice([-1.0, 1.0], size=len(rows))
            st.params[name] = w
        elif leaf == "gamma":
            st.params[name] = rng.choice([1.0, 2.0], size=v.shape).astype(np.float32)
        else:
            st.params[name] = rng.integers(-3, 4, size=v.shape).astype(np.float32)
    for name, v in list(st.moving.items()):
        st.moving[name] = (np.full(v.shape, 0.999, np.float32) if name.endswith("moving_variance")
                           else rng.integers(-3, 4, size=v.shape).astype(np.float32))
    return cfg, st


def integer_inputs(B, seed=1, dim=32):
    return np.random.default_rng(seed).integers(-4, 5, size=(B, dim)).astype(np.float32)


def integer_dy(B, D, seed=2):
    """An output gradient of float32 integers in [-2, 2] (p3d_backward takes the caller's dy)."""
    return np.random.default_rng(seed).integers(-2, 3, size=(B, D)).astype(np.float32)


EXACT_LIMIT = 2.0 ** 23   # below it every integer, and every partial sum of integers, is a float32


def _abs_bounds(st, cache, dy):
    """For every linear layer of a no-BN model, the largest sum of absolute values of each of its
    contractions in the training forward and the backward: |x| |W| + |b| (z), |x|^T |dz| (dW),
    sum |dz| (db), |dz| |W|^T (dx), and the residual adds.  Any partial sum of a contraction, in any
    order, tiling or split, is at most this in magnitude.  The walk repeats ref_mlp.backward for
    layers without BN (float64, exact on integers) and is checked against it by the caller."""
    P = {k: np.abs(v.astype(np.float64)) for k, v in st.params.items()}
    bounds, dws = {}, {}

    def lin(tag, wname, bname, x, dz):
        ax, adz = np.abs(x.astype(np.float64)), np.abs(dz)
        bounds[tag] = {"z": float((ax @ P[wname] + P[bname]).max()), "dW": float((ax.T @ adz).max()),
                       "db": float(adz.sum(axis=0).max()), "dx": float((adz @ P[wname].T).max())}
        dws[wname] = x.astype(np.float64).T @ dz
        return dz @ st.params[wname].astype(np.float64).T

    def layer(key, dout):
        rec = cache[key]
        g = dout
        if rec["keep"] < 1.0:
            g = (g * rec["mask"]) / np.float64(rec["keep"])
        return lin(key, rec["wname"], rec["bname"], rec["x"], g * (rec["a"] > 0))

    dh = lin("out", "linear_model/w4", "linear_model/b4", cache["out"]["x"], dy.astype(np.float64))
    for i in reversed(range(st.cfg.num_layers)):
        dout = dh
        dh = layer("A%d" % i, layer("B%d" % i, dout))
        if st.cfg.residual:
            bounds["res%d" % i] = {"dx": float((np.abs(dh) + np.abs(dout)).max())}
            dh = dh + dout
    layer("in", dh)
    return bounds, dws


def exact_backward(st, x, dy, keep, seed, ctr, row0):
    """The oracle's float32 training forward and backward (dropout at `keep` from the Philox stream
    the kernels share, keyed by seed / ctr / row0) with the checks that they ARE exact: float32 and
    float64 agree bit for bit on the outputs and on every gradient, every gradient is an integer,
    and the sum of absolute values of every contraction (_abs_bounds) stays below 2^23 -- so any
    summation order, tiling, K split or batch split gives these bits.  keep must make the dropout
    scale exact (1 or a power of two).  Models with BN or max-norm are refused: 1 / sqrt(var + eps)
    and the Frobenius norm are not exact.  Returns (outputs, {name: gradient}) in float32."""
    cfg = st.cfg
    assert not cfg.batch_norm and not cfg.max_norm, "exact_backward: BN and max-norm are not exact"
    assert np.log2(keep) == np.round(np.log2(keep)), "exact_backward: 1 / keep must be a power of two"
    for v in (x, dy):
        assert v.dtype == np.float32 and np.array_equal(v, np.round(v)), "integer inputs only"
    res = {}
    for dt in (np.float32, np.float64):
        out, cache = ref_mlp.forward(st, x, True, keep, seed, ctr, row0, dt=dt)
        res[dt] = (out, ref_mlp.backward(st, cache, dy.astype(dt), dt=dt), cache)
    (out, grads, cache), (out64, grads64, cache64) = res[np.float32], res[np.float64]
    assert out.dtype == np.float32 and np.array_equal(out, out64), "outputs differ between float32 and float64"
    assert sorted(grads) == sorted(n for n, _ in ref_mlp.param_names(cfg))
    for name, g in grads.items():
        assert g.dtype == np.float32, name
        assert np.array_equal(g, grads64[name]), "%s differs between float32 and float64" % name
        assert np.array_equal(g, np.round(g)), "%s is not an integer gradient" % name
    bounds, dws = _abs_bounds(st, cache64, dy)
    for wname, dw in dws.items():   # (the bounds were taken on the oracle's own dz)
        assert np.array_equal(dw, grads64[wname]), wname
    worst = max(v for b in bounds.values() for v in b.values())
    assert worst < EXACT_LIMIT, "a contraction's absolute sum %g leaves float32's exact range" % worst
    return out, grads


# The shapes of the exact training tests (tests/test_gpu_exact.py on the GPU, and
# tests/test_oracle.py for the proof that each is exact): name -> (L, blocks, residual, predict_14,
# B, keep, row0).  cfg3's shape at keep 1 and 0.5; ragged row tiles (17, 37); more than one
# 64-row tile (200); a narrow model without residual; a data-parallel rank's row offset into the
# dropout key; the 42 outputs of --predict_14.
BACKWARD_CASES = {
    "cfg3_keep1": (1024, 2, True, False, 64, 1.0, 0),
    "cfg3_keep05": (1024, 2, True, False, 64, 0.5, 0),
    "b17": (1024, 2, True, False, 17, 0.5, 0),
    "b37": (1024, 2, True, False, 37, 0.5, 0),
    "b200": (1024, 2, True, False, 200, 0.5, 0),
    "l256_nores": (256, 2, False, False, 17, 0.5, 0),
    "row_offset": (1024, 2, True, False, 64, 0.5, 3 * 64),
    "predict_14": (1024, 2, True, True, 37, 0.5, 0),
}
BACKWARD_SEED, BACKWARD_CTR = 3, 7   # the model seed and the call counter of the dropout key
_backward_cache = {}


def backward_case(name):
    """(cfg, st, x, dy, keep, row0, out, grads) of BACKWARD_CASES[name]; computed once per process
    and shared (read-only arrays)."""
    if name not in _backward_cache:
        L, N, residual, p14, B, keep, row0 = BACKWARD_CASES[name]
        cfg, st = integer_state(L, N, nnz=8, residual=residual, batch_norm=False, predict_14=p14)
        x = integer_inputs(B, seed=300 + B)
        dy = integer_dy(B, cfg.output_size, seed=400 + B)
        out, grads = exact_backward(st, x, dy, keep, BACKWARD_SEED, BACKWARD_CTR, row0)
        for a in [x, dy, out, *grads.values()]:
            a.setflags(write=False)
        _backward_cache[name] = (cfg, st, x, dy, keep, row0, out, grads)
    return _backward_cache[name]


def exact_forward(st, x):
    """The oracle's float32 forward, with the check that it IS exact: every pre-activation,
    activation and output an integer of magnitude < 2^23."""
    out, cache = ref_mlp.forward(st, x, False, dt=np.float32)
    vals = [cache[k][f] for k in cache if k not in ("order", "out") for f in ("z", "a")] + [out]
    for v in vals:
        assert np.array_equal(v, np.round(v)), "not an integer model"
        assert float(np.abs(v).max()) < 2.0 ** 23, "integer model leaves float32's exact range"
    return out
