"""CPU-side proofs for tests/shape_cases.py (no GPU): every integer case of the shape tables is exact,
none is blind to a dropped k-group, the layout formula equals the library's, the tables reach every
layout and every launch form on both sides of each threshold, and the boundary of what
p3d_vae_create accepts is where VAE_REFUSED says."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _p3d  # noqa: E402
import exact_models  # noqa: E402
import shape_cases as sc  # noqa: E402
import vae_exact as ve  # noqa: E402
import vae_oracle as vo  # noqa: E402
from oracle import ref_mlp  # noqa: E402


# ---- the lifter's integer cases -------------------------------------------------------------------
def _with_weight(st, wname, w):
    st2 = st.copy()
    st2.params[wname] = w
    return st2


@pytest.mark.parametrize("name", list(sc.LIFTER_SHAPES))
def test_lifter_forward_cases_are_exact_and_see_every_kgroup(name):
    """exact_forward at B = 70 (and, for the shapes it is cheap for, at every batch the GPU tests
    run); with one 16-row k-group of a layer's weights zeroed the output changes, for every layer."""
    cfg, st, x, out = sc.lifter_exact_case(name, 70)
    for wname in sc.weight_names(cfg):
        st2 = _with_weight(st, wname, sc.drop_kgroup(st.params[wname]))
        out2, _ = ref_mlp.forward(st2, x, False, dt=np.float32)
        assert not np.array_equal(out2, out), "%s: blind to a dropped k-group of %s" % (name, wname)
    batches = set(sc.forward_batches(name))
    if sc.serve_expected(cfg, 64) == "runs":
        batches |= set(sc.SERVE_BATCHES)
    for B in sorted(batches):
        sc.lifter_exact_case(name, B)


@pytest.mark.parametrize("run", sc.backward_runs(), ids=lambda r: "%s-B%d-row%d" % (r[0], r[1], r[3]))
def test_lifter_backward_cases_are_exact_and_see_every_kgroup(run):
    """exact_backward on the no-BN twin at the batches the GPU test uses (nnz 8 up to three blocks,
    2 beyond); with one k-group of a layer zeroed the training outputs change for every layer and at
    least one gradient does."""
    name = run[0]
    cfg, st, x, dy, keep, row0, out, grads = sc.lifter_backward_case(*run)
    assert sc.backward_nnz(name) == (8 if cfg.num_layers <= 3 else 2) and not cfg.batch_norm
    seed, ctr = exact_models.BACKWARD_SEED, exact_models.BACKWARD_CTR
    for wname in sc.weight_names(cfg):
        st2 = _with_weight(st, wname, sc.drop_kgroup(st.params[wname]))
        out2, cache = ref_mlp.forward(st2, x, True, keep, seed, ctr, row0, dt=np.float32)
        assert not np.array_equal(out2, out), "%s: outputs blind to a dropped k-group of %s" % (name, wname)
        g2 = ref_mlp.backward(st2, cache, dy, dt=np.float32)
        assert any(not np.array_equal(g2[n], grads[n]) for n in grads), (name, wname)


def test_deep_twins_need_the_sparser_weights():
    """The pairing the table keeps: with 8 non-zeros per column the 7- and 8-block models leave
    float32's exact range in the forward, and the 8-block twin in the backward."""
    for name in ("L128_N7", "L128_N8"):
        L, N, residual, bn, nnz, _ = sc.LIFTER_SHAPES[name]
        assert nnz == 2
        _, st = exact_models.integer_state(L, N, nnz=8, residual=residual, batch_norm=bn)
        with pytest.raises(AssertionError, match="exact range"):
            exact_models.exact_forward(st, exact_models.integer_inputs(70, seed=770))
    _, st = exact_models.integer_state(128, 8, nnz=8, residual=True, batch_norm=False)
    with pytest.raises(AssertionError):
        exact_models.exact_backward(st, exact_models.integer_inputs(64, seed=364), exact_models.integer_dy(64, 48, seed=464),
                                    0.5, exact_models.BACKWARD_SEED, exact_models.BACKWARD_CTR, 0)


# ---- the filter's integer cases ---------------------------------------------------------------------
@pytest.mark.parametrize("B", sc.VAE_EXACT_BATCHES)
@pytest.mark.parametrize("name", sc.vae_exact_names())
def test_vae_cases_are_exact_and_see_every_kgroup(name, B):
    shape = sc.VAE_SHAPES[name]
    k = ve.exact_case(B, shape)
    for wname in sc.vae_kernel_names(shape):
        P = dict(k["P"])
        P[wname] = sc.drop_kgroup(P[wname])
        c = vo.forward(P, shape, k["x"], k["eps"], np.float32)
        assert not np.array_equal(c["y"], k["y"]), "%s: y blind to a dropped k-group of %s" % (name, wname)
        g, _ = vo.backward(P, shape, c, k["t"], k["factors"], np.float32)
        assert any(not np.array_equal(g[n], k["grads"][n]) for n in g), (name, wname)


# ---- the layout formula -----------------------------------------------------------------------------
def _lds(shape):
    i, enc, lat, dec, out = shape
    e, d = (ctypes.c_int32 * len(enc))(*enc), (ctypes.c_int32 * len(dec))(*dec)
    return int(_p3d.lib().p3d_vae_lds_bytes(i, len(enc), e, lat, len(dec), d, out))


def _seq_lds(shape, form):
    i, enc, lat, dec, out = shape
    e, d = (ctypes.c_int32 * len(enc))(*enc), (ctypes.c_int32 * len(dec))(*dec)
    return int(_p3d.lib().p3d_vae_seq_lds_bytes(i, len(enc), e, lat, len(dec), d, out, form))


def _existing_shapes():
    import test_gpu_vae
    import test_gpu_vae_seq
    import test_gpu_vae_wide
    return {m.__name__ + ":" + n: s for m in (test_gpu_vae, test_gpu_vae_seq, test_gpu_vae_wide) for n, s in m.SHAPES.items()}


def test_layout_formula_equals_the_library():
    """vae_layout_bytes at the first try that fits == p3d_vae_lds_bytes (vae_plan of
    csrc/p3d_vae_layout.h, restated independently in shape_cases), for every table entry and
    every shape of the existing GPU tests; the table's indices and sizes are the recorded ones."""
    assert sorted(sc.VAE_LAYOUT) == sorted(sc.VAE_SHAPES)
    for name, shape in sc.VAE_SHAPES.items():
        idx, nbytes = sc.VAE_LAYOUT[name]
        assert sc.vae_layout_index(shape) == idx, name
        assert sc.vae_best_bytes(shape) == nbytes == _lds(shape), name
        assert nbytes <= sc.VAE_LDS_LIMIT
        for i in range(idx):                       # the roomier tries do not fit
            assert sc.vae_layout_bytes(shape, *sc.VAE_TRIES[i]) > sc.VAE_LDS_LIMIT, (name, i)
    existing = _existing_shapes()
    assert len(existing) >= 9
    for name, shape in existing.items():
        assert sc.vae_best_bytes(shape) == _lds(shape), name
    # DESIGN 5h's example: the 144-input default shape fits with the stagger, without the input tile
    s144 = (144, (40, 32), 24, (32, 40), 48)
    assert sc.vae_layout_index(s144) == 1 and sc.vae_best_bytes(s144) == 161664 == _lds(s144)


def test_tables_reach_every_layout_and_the_existing_tests_do_not():
    assert {i for i, _ in sc.VAE_LAYOUT.values()} == {0, 1, 2}
    narrow = [s for n, s in _existing_shapes().items() if s[0] <= 256]
    assert 2 not in {sc.vae_layout_index(s) for s in narrow}


def test_sequence_filter_serves_the_listed_entries():
    for name, shape in sc.VAE_SHAPES.items():
        for form in (0, 1):
            assert (_seq_lds(shape, form) > 0) == (name in sc.VAE_SEQ_NAMES), (name, form)


def test_boundary_of_acceptance():
    """From w136_edge (448 B under the limit) one hidden width is raised in steps of 8 until no
    layout fits: the fewest steps lead to VAE_REFUSED, whose size is the committed one; the
    encoder width 144 still fits, in the second layout."""
    base = sc.VAE_SHAPES["w136_edge"]
    assert sc.VAE_LDS_LIMIT - _lds(base) == 448
    s144 = (48, (144,), 8, (64,), 48)
    assert _lds(s144) == 151232 and sc.vae_layout_index(s144) == 1
    found = []
    for side in ("enc", "dec"):
        w0 = base[1][0] if side == "enc" else base[3][0]
        for steps, w in enumerate(range(w0 + 8, 257, 8), 1):
            shape = (base[0], (w,), base[2], base[3], base[4]) if side == "enc" else (base[0], base[1], base[2], (w,), base[4])
            if _lds(shape) > sc.VAE_LDS_LIMIT:
                assert all(sc.vae_layout_bytes(shape, *t) > sc.VAE_LDS_LIMIT for t in sc.VAE_TRIES)
                found.append((steps, shape, _lds(shape)))
                break
    steps, shape, nbytes = min(found)
    assert (shape, nbytes) == sc.VAE_REFUSED and steps == 5
    assert nbytes == sc.vae_layout_bytes(shape, 0, 0)


# ---- the launch forms the tables reach ------------------------------------------------------------
def test_tables_reach_every_launch_form():
    """Over LIFTER_SHAPES x the GPU tests' batches on 256 compute units, the union of the expected
    tags holds both sides of every threshold."""
    fwd, train, bwd, serve = set(), set(), set(), set()
    for name in sc.LIFTER_SHAPES:
        cfg = sc.lifter_cfg(name)
        for B in sc.forward_batches(name):
            fwd |= set(sc.expected_forward_tags(cfg, B, sc.REF_CUS))
            serve.add(sc.serve_expected(cfg, B))
    for name, B in sc.bn_runs():
        cfg = sc.lifter_cfg(name, batch_norm=True)
        train |= set(sc.expected_forward_tags(cfg, B, sc.REF_CUS, training="step"))
        bwd |= set(sc.expected_backward_tags(cfg, B, sc.REF_CUS))
    for name, B, _, _ in sc.backward_runs():
        bwd |= set(sc.expected_backward_tags(sc.lifter_cfg(name, batch_norm=False), B, sc.REF_CUS))
    assert {"gemv_chain", "gemv_in_hidden", "gemv_hidden_out", "gemv_in", "gemv_hidden", "gemv_out"} <= fwd
    assert {"fwd_in", "fwd_in_big", "fwd_hidden", "fwd_hidden_big", "fwd_out"} <= fwd
    assert {"fwd_out_part", "fwd_out_train", "fwd_hidden_train_x", "fwd_hidden_train_z", "bn_fwd"} <= train
    assert {"wgrad_multi", "wgrad", "dgrad_out", "dgrad_hidden", "bn_bwd"} <= bwd
    assert serve == {"runs", "refused"}


def test_expected_tags_on_the_thresholds():
    """Spot checks of the restated conditions, each against the sentence of csrc/p3d.hip it restates."""
    c = sc.lifter_cfg
    assert sc.expected_forward_tags(c("L256_N4"), 4, 256) == {"gemv_chain": 1}                # H = 8, 8 x 16 tiles
    assert sc.expected_forward_tags(c("L256_N4"), 4, 120) == {"gemv_in_hidden": 1, "gemv_hidden": 6, "gemv_hidden_out": 1}
    assert sc.expected_forward_tags(c("L256_N5"), 1, 256) == {"gemv_in_hidden": 1, "gemv_hidden": 8, "gemv_hidden_out": 1}
    assert sc.expected_forward_tags(c("L2112_N1"), 1, 256) == {"gemv_in_hidden": 1, "gemv_hidden_out": 1}
    assert sc.expected_forward_tags(c("L4160_N1"), 1, 256) == {"gemv_in": 1, "gemv_hidden": 2, "gemv_out": 1}
    assert sc.expected_forward_tags(c("L64_N0"), 4, 256) == {"gemv_in": 1, "gemv_out": 1}
    assert sc.expected_forward_tags(c("L64_N0"), 5, 256) == {"fwd_in": 1, "fwd_out": 1}
    assert sc.expected_forward_tags(c("L128_N3"), 300, 256) == {"fwd_in_big": 1, "fwd_hidden_big": 6, "fwd_out": 1}
    assert sc.expected_forward_tags(c("L192_N2"), 300, 256) == {"fwd_in_big": 1, "fwd_hidden": 4, "fwd_out": 1}
    assert sc.expected_forward_tags(c("L128_N3"), 65, 256) == {"fwd_in": 1, "fwd_hidden": 6, "fwd_out": 1}
    assert sc.expected_forward_tags(c("L64_N0"), 64, 256, "step") == {"fwd_in_train_x": 1, "fwd_out_train": 1}
    assert sc.expected_forward_tags(c("L64_N1"), 256, 256, "step") == {"fwd_in_train_x": 1, "fwd_hidden_train_x": 2,
                                                                         "fwd_out_part": 1}
    assert sc.expected_forward_tags(c("L64_N1"), 257, 256, "step") == {"fwd_in_train_z": 1, "fwd_hidden_train_z": 2,
                                                                         "bn_fwd": 3, "fwd_out_train": 1}
    assert sc.expected_backward_tags(c("L128_N7", False), 64, 256) == {"dgrad_out": 1, "dgrad_hidden": 14, "wgrad_multi": 1}
    assert sc.expected_backward_tags(c("L128_N8", False), 64, 256) == {"dgrad_out": 1, "dgrad_hidden": 16, "wgrad": 18}
    assert sc.expected_backward_tags(c("L64_N0", False), 17, 256) == {"dgrad_out": 1, "wgrad_multi": 1}
    assert sc.expected_backward_tags(c("L64_N1"), 257, 256) == {"dgrad_out": 1, "dgrad_hidden": 2, "bn_bwd": 3, "wgrad_multi": 1}


def test_serve_expected_equals_the_planner():
    """serve_expected against p3d_serve_plan (host only) on 256 compute units: a shape it calls
    "refused" is refused with the documented message, one it calls "runs" gets a kernel at every
    batch of the GPU test."""
    lib = _p3d.lib()
    for name in sc.LIFTER_SHAPES:
        cfg = sc.lifter_cfg(name)
        pcfg = _p3d.P3DCfg(cfg.linear_size, cfg.num_layers, int(cfg.residual), int(cfg.batch_norm), 0, 32, 48,
                           _p3d.P3D_DTYPE_F32, 64, 1e-3, 0.99)
        for B in sc.SERVE_BATCHES:
            planned = ctypes.create_string_buffer(128)
            rc = lib.p3d_serve_plan(ctypes.byref(pcfg), sc.REF_CUS, B, 0, planned, 128, None)
            if sc.serve_expected(cfg, B) == "refused":
                assert rc == _p3d.P3D_ERR_ARG and lib.p3d_last_error().decode() == sc.SERVE_REFUSAL, (name, B)
            else:
                assert rc == 0 and planned.value.startswith(b"k_serve"), (name, B, rc, lib.p3d_last_error())
