"""Bit-exact parity of the inference paths against the oracle at full size (tests/exact_models.py:
integer-valued models, for which float32 and the bf16 emulation are exact whatever the summation
order).  Every launch form the library picks for a batch size is covered: the persistent forms of
p3d_serve (k_serve6: the 20-request headline's pair form, a lone batch-64 request, ragged row
counts; k_serve5: long launches), the per-layer kernel chain (k_fwd), the batch <= 4 persistent
GEMV chain (k_gemv_chain), the large-M GEMM (k_gemm_f32) and the cfg5 bf16 GEMMs (k_gemm_bf16p).

The training side (second half): the training forward with dropout and p3d_backward on integer
models without BN, every trainable's gradient equal to the oracle's bit for bit, through each dy
entry path and each launch form of the backward (k_dgrad's built instantiations, the one-launch and
bucketed k_wgrad_grad, the per-layer k_wgrad)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_models  # noqa: E402
import linear_model  # noqa: E402
from oracle import ref_mlp  # noqa: E402


def _model(cfg, st, max_batch, dtype=None):
    kw = {"dtype": dtype} if dtype else {}
    m = linear_model.LinearModel(cfg.linear_size, cfg.num_layers, cfg.residual, cfg.batch_norm, False, 64, 1e-3,
                                 "/tmp/p3d_exact", cfg.predict_14, seed=3, max_batch=max_batch, **kw)
    m.set_weights({**st.params, **st.moving})
    return m


@pytest.fixture(scope="module")
def cfg2():
    cfg, st = exact_models.integer_state(1024, 2, nnz=8)
    return cfg, st


@pytest.mark.parametrize("B", [1280, 1217, 64, 37, 64 * 300 + 13])
def test_serve_bit_exact(cfg2, B):
    """p3d_serve (1280 rows = the driver's 20-request launch: k_serve6's pair form; 1217 ragged;
    64 = one request; 37; 19,213 rows = k_serve5) == the oracle, bit for bit."""
    cfg, st = cfg2
    x = exact_models.integer_inputs(B, seed=B)
    ref = exact_models.exact_forward(st, x)
    m = _model(cfg, st, max_batch=64)
    y = m.serve_device(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    m.serve_check()
    np.testing.assert_array_equal(y.cpu().numpy(), ref)
    m.close()


@pytest.mark.parametrize("B", [1, 3, 4, 37, 64, 300, 4096])
def test_forward_bit_exact(cfg2, B):
    """forward_device (B <= 4: k_gemv_chain; B <= 64: the per-layer k_fwd chain; B >= 256: the
    large-M k_gemm_f32) == the oracle, bit for bit."""
    cfg, st = cfg2
    x = exact_models.integer_inputs(B, seed=100 + B)
    ref = exact_models.exact_forward(st, x)
    m = _model(cfg, st, max_batch=max(B, 64))
    y = m.forward_device(torch.from_numpy(x).cuda())
    np.testing.assert_array_equal(y.cpu().numpy(), ref)
    m.close()


@pytest.mark.parametrize("residual,batch_norm,p14", [(False, True, False), (True, False, False), (True, True, True)])
def test_flag_variants_bit_exact(residual, batch_norm, p14):
    """Flag combinations (no residual, no BN, --predict_14's 42 outputs) through p3d_serve and the
    kernel chain, bit for bit."""
    cfg, st = exact_models.integer_state(1024, 2, nnz=8, residual=residual, batch_norm=batch_norm, predict_14=p14)
    x = exact_models.integer_inputs(1280, seed=9)
    ref = exact_models.exact_forward(st, x)
    m = _model(cfg, st, max_batch=64)
    if cfg.output_size == 48:   # (p3d_serve's persistent forms are built for 48 outputs)
        y = m.serve_device(torch.from_numpy(x).cuda())
        torch.cuda.synchronize()
        m.serve_check()
        np.testing.assert_array_equal(y.cpu().numpy(), ref)
    y = torch.cat([m.forward_device(torch.from_numpy(x[i:i + 64]).cuda()) for i in range(0, 1280, 64)])
    np.testing.assert_array_equal(y.cpu().numpy(), ref)
    m.close()


@pytest.mark.parametrize("L,N,B,nnz", [(4096, 4, 1024, 4), (1024, 2, 256, 8), (512, 1, 200, 8)])
def test_bf16_bit_exact(L, N, B, nnz):
    """cfg5's bf16 path (BASELINE configs[4] at full size: L = 4096, 4 blocks, B = 1024) == the
    oracle's bf16 emulation, bit for bit (replaces a 1 %-of-range bound)."""
    cfg, st = exact_models.integer_state(L, N, nnz=nnz)
    x = exact_models.integer_inputs(B, seed=L + B)
    exact_models.exact_forward(st, x)                       # (the model is exact in float32)
    ref = ref_mlp.forward_bf16(st, x, acc=np.float64)
    assert np.array_equal(ref, ref_mlp.forward_bf16(st, x, acc=np.float32))   # order-independent
    m = _model(cfg, st, max_batch=B, dtype="bfloat16")
    y = m.forward_device(torch.from_numpy(x).cuda())
    np.testing.assert_array_equal(y.cpu().numpy(), ref)
    m.close()


# ---- training: the forward with dropout and p3d_backward, bit for bit (exact_models.exact_backward) ----
# dy entry paths of p3d_backward: a 48-wide dy at a 16-byte aligned pointer is read in place; any
# other (42 outputs, or a pointer off by one float) goes through the zero-padded copy.

def _tags(m, fn):
    """The kernel tags p3d_profile_start / stop saw while fn ran: {tag: launches}."""
    import ctypes
    import _p3d
    _p3d.check(_p3d.lib().p3d_profile_start(m._h, 64), "p3d_profile_start")
    fn()
    buf = ctypes.create_string_buffer(1 << 12)
    _p3d.check(_p3d.lib().p3d_profile_stop(m._h, buf, len(buf)), "p3d_profile_stop")
    return {ln.split("\t")[0]: int(ln.split("\t")[1]) for ln in buf.value.decode().strip().splitlines()}


def _train_model(cfg, st, max_batch=64):
    m = linear_model.LinearModel(cfg.linear_size, cfg.num_layers, cfg.residual, cfg.batch_norm, False, 64, 1e-3,
                                 "/tmp/p3d_exact", cfg.predict_14, seed=exact_models.BACKWARD_SEED,
                                 max_batch=max_batch)
    m.set_weights({**st.params, **st.moving})
    return m


def _exact_step(m, case, misalign=False, poison=False):
    """One training forward + p3d_backward of a BACKWARD_CASES entry on model m, everything compared
    with the oracle by assert_array_equal: the outputs, every trainable's gradient, and the caller's
    dy left as it was.  Returns the tags of the backward's launches.  poison: the flat gradient
    buffer is NaN beforehand, so an element the backward does not write (or adds to) shows."""
    import _p3d
    cfg, st, x, dy, keep, row0, out, grads = exact_models.backward_case(case)
    B, D = dy.shape
    xd = torch.tensor(x).cuda()                       # (the library differentiates this buffer: held)
    if misalign:                                      # a view one float into a larger buffer
        buf = torch.zeros(B * D + 8, dtype=torch.float32, device="cuda")
        dyd = buf[1:1 + B * D].view(B, D)
        dyd.copy_(torch.tensor(dy))
        assert dyd.data_ptr() % 16 == 4
    else:
        dyd = torch.tensor(dy).cuda()
        assert dyd.data_ptr() % 16 == 0
    if poison:
        m.flat["grads"].fill_(float("nan"))
    y = m.forward_device(xd, True, keep, ctr=exact_models.BACKWARD_CTR, row_offset=row0)
    np.testing.assert_array_equal(y.cpu().numpy(), out, err_msg="%s: training forward" % case)
    tags = _tags(m, lambda: _p3d.check(_p3d.lib().p3d_backward(m._h, _p3d.ptr(dyd), B, m.stream()), "p3d_backward"))
    torch.cuda.synchronize()
    assert sorted(m.trainable_names()) == sorted(grads)
    for name in m.trainable_names():
        np.testing.assert_array_equal(m.grad(name).cpu().numpy(), grads[name], err_msg="%s: %s" % (case, name))
    np.testing.assert_array_equal(dyd.cpu().numpy(), dy, err_msg="%s: dy was written" % case)
    m.check_errors()
    return tags


def _default_tags(cfg):
    """p3d_backward's default form: the data gradient of the output layer and of every hidden
    layer, then every layer's weight gradient in ONE gradient-only launch (k_wgrad_grad)."""
    return {"dgrad_out": 1, "dgrad_hidden": 2 * cfg.num_layers, "wgrad_multi": 1}


@pytest.mark.parametrize("case", sorted(exact_models.BACKWARD_CASES))
def test_backward_bit_exact(case):
    """Training forward (dropout from the shared Philox stream) and p3d_backward on the integer
    no-BN models == the oracle, bit for bit, for every trainable: cfg3's shape at keep 1 and 0.5,
    ragged row tiles (B = 17, 37), B = 200 (four 64-row slices of each weight-gradient tile's
    contraction, 13 row tiles of the data gradient), L = 256 without residual, a data-parallel
    rank's row offset in the mask key, and --predict_14 (42 outputs: dy through the padded copy).
    Run twice on one model, the second time over a NaN-filled gradient buffer: the same bits."""
    cfg, st = exact_models.backward_case(case)[:2]
    m = _train_model(cfg, st, max_batch=max(64, exact_models.BACKWARD_CASES[case][4]))
    assert _exact_step(m, case) == _default_tags(cfg)
    assert _exact_step(m, case, poison=True) == _default_tags(cfg)
    m.close()


def test_backward_bit_exact_unaligned_dy():
    """A 48-wide dy whose pointer is not 16-byte aligned (a view one float into a buffer) takes the
    padded copy instead of being read in place: the same gradients, bit for bit."""
    cfg, st = exact_models.backward_case("cfg3_keep05")[:2]
    m = _train_model(cfg, st)
    assert _exact_step(m, "cfg3_keep05", misalign=True) == _default_tags(cfg)
    assert _exact_step(m, "b37", misalign=True) == _default_tags(cfg)
    m.close()


def test_backward_bit_exact_across_calls():
    """One model, calls of different batch, keep, row offset and dy path in turn, then the first
    again: every call's bits are the oracle's, so nothing (a cached batch, a mask key, a padded dy
    row, a flag of the split form) is carried from one call into the next."""
    cfg, st = exact_models.backward_case("cfg3_keep05")[:2]
    m = _train_model(cfg, st, max_batch=200)
    for i, case in enumerate(["cfg3_keep05", "b200", "b17", "cfg3_keep1", "row_offset", "b37", "cfg3_keep05"]):
        assert _exact_step(m, case, misalign=(i % 3 == 2), poison=True) == _default_tags(cfg), case
    m.close()


def _two_buckets(m):
    """The data-parallel plan of two all-reduce buckets (dist_utils.plan_buckets over the layers'
    flat gradient ranges at 8 MB, LinearModel.dp_buckets' arithmetic), set through p3d_grad_buckets."""
    import ctypes
    import _p3d
    import dist_utils
    ranges = []
    for l in range(2 * m.num_layers + 2):
        b, e = ctypes.c_int64(), ctypes.c_int64()
        _p3d.check(_p3d.lib().p3d_layer_grad_range(m._h, l, ctypes.byref(b), ctypes.byref(e)), "p3d_layer_grad_range")
        ranges.append((b.value, e.value))
    plan = dist_utils.plan_buckets(ranges, (8 << 20) // 4)
    assert len(plan) == 2, plan
    lo = (ctypes.c_int32 * len(plan))(*[b[2] for b in plan])
    _p3d.check(_p3d.lib().p3d_grad_buckets(m._h, len(plan), lo), "p3d_grad_buckets")


def _layer_buckets(m):
    import _p3d
    _p3d.check(_p3d.lib().p3d_grad_events(m._h, 1), "p3d_grad_events")


# form -> (environment at p3d_create, set-up on the model, the backward's tags at 2 blocks)
_FORMS = {
    # the per-layer weight-gradient kernel k_wgrad, one launch per layer
    "wgrad_per_layer": ({"P3D_WGRAD_MULTI": "0"}, None, {"dgrad_out": 1, "dgrad_hidden": 4, "wgrad": 6}),
    # the whole-batch data-gradient kernels (one workgroup owns all rows of its 16 columns)
    "whole_batch": ({"P3D_TRAIN_SPLIT": "0"}, None, {"dgrad_out": 1, "dgrad_hidden": 4, "wgrad_multi": 1}),
    # one gradient bucket per layer: six k_wgrad_grad launches, each behind its layer's dZ
    "bucket_per_layer": ({}, _layer_buckets, {"dgrad_out": 1, "dgrad_hidden": 4, "wgrad_bucket": 6}),
    # the data-parallel form's two buckets: {output, hidden 4, hidden 3} and {hidden 2, hidden 1, input}
    "two_buckets": ({}, _two_buckets, {"dgrad_out": 1, "dgrad_hidden": 4, "wgrad_bucket": 2}),
    # the other built k_dgrad instantiations: 8 waves for the hidden layers (default 16), 8 waves
    # for the output layer's (default 4); the tags do not tell instantiations apart
    "dgrad_8_waves": ({"P3D_DGRAD_WK": "8", "P3D_DGRAD_OUT_WK": "8"}, None,
                      {"dgrad_out": 1, "dgrad_hidden": 4, "wgrad_multi": 1}),
}


@pytest.mark.parametrize("case", ["cfg3_keep05", "b37"])
@pytest.mark.parametrize("form", sorted(_FORMS))
def test_backward_forms_bit_exact(form, case, monkeypatch):
    """The alternative launch forms of p3d_backward against the ORACLE (they were compared with each
    other only): cfg3's shape at keep 0.5, B = 64 and the ragged B = 37, through the per-layer k_wgrad,
    the whole-batch kernels, per-layer and two-bucket k_wgrad_grad launches and the 8-wave k_dgrad
    instantiations -- the tags say which weight-gradient form ran -- twice on one model."""
    env, setup, want = _FORMS[form]
    for k in ("P3D_WGRAD_MULTI", "P3D_TRAIN_SPLIT", "P3D_DGRAD_WK", "P3D_DGRAD_OUT_WK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, st = exact_models.backward_case(case)[:2]
    m = _train_model(cfg, st, max_batch=128)
    if setup:
        setup(m)
    assert _exact_step(m, case) == want
    assert _exact_step(m, case, poison=True) == want
    if form == "whole_batch":
        # the environment reached the model: this form refuses a batch above 64 before any launch
        import _p3d
        xd = torch.zeros((65, 32), device="cuda")
        m.forward_device(xd, True, 1.0, ctr=0, row_offset=0)
        dyd = torch.zeros((65, 48), device="cuda")
        assert _p3d.lib().p3d_backward(m._h, _p3d.ptr(dyd), 65, m.stream()) == _p3d.P3D_ERR_ARG
        assert b"P3D_TRAIN_SPLIT=0" in _p3d.lib().p3d_last_error()
        torch.cuda.synchronize()
    m.close()
