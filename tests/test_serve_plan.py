"""The serve planner (csrc/p3d_serve_plan.h) through p3d_serve_plan, without a GPU: which kernel a
p3d_serve / p3d_serve_mse launch runs is a pure function of (model shape, CU count, P3D_SERVE6*
knobs, batch, with-loss).

tests/golden/serve_plan_parent.json holds answers of the selection code as it stood inside
serve_impl before the planner existed (sampled over widths, blocks, output sizes, CU counts, batches
and knob sets); every row must reproduce.  The anchors pin the cases the design documents speak of."""
import ctypes
import json
import os
import sys

import pytest

import _p3d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "serve_plan_parent.json")
KNOBS = ("P3D_SERVE6", "P3D_SERVE6_MAX_NB", "P3D_SERVE6_SPLIT", "P3D_SERVE6_RT", "P3D_SERVE6_DEPTH",
         "P3D_SERVE6_PAIR", "P3D_SERVE6_ROUNDS")
ROUNDS = "k_serve6_rounds<4, 3, 2, 5>"


def plan(monkeypatch, B, env="", L=1024, num_layers=2, output_size=48, cus=256, with_loss=0):
    """(name, [S, rt, ncm, depth, nb]) of the launch, or None where it is refused with P3D_ERR_ARG."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for kv in env.split():
        k, v = kv.split("=")   # "P3D_SERVE6_SPLIT=3", or short: "SPLIT=3", "SERVE6=2"
        if not k.startswith("P3D_"):
            k = "P3D_SERVE6" if k == "SERVE6" else "P3D_SERVE6_" + k
        assert k in KNOBS, k
        monkeypatch.setenv(k, v)
    cfg = _p3d.P3DCfg(L, num_layers, 1, 1, 0, 32, output_size, _p3d.P3D_DTYPE_F32, 64, 1e-3, 0.99)
    name = ctypes.create_string_buffer(128)
    shape = (ctypes.c_int32 * 5)()
    rc = _p3d.lib().p3d_serve_plan(ctypes.byref(cfg), cus, B, with_loss, name, 128, shape)
    if rc == _p3d.P3D_ERR_ARG:
        return None
    assert rc == 0, _p3d.lib().p3d_last_error()
    return name.value.decode(), list(shape)


@pytest.fixture(scope="module")
def table():
    with open(GOLD) as f:
        return json.load(f)


def test_table_of_the_parents_answers_reproduces(monkeypatch, table):
    assert len(table) >= 300
    bad = []
    for r in table:
        got = plan(monkeypatch, r["B"], r["env"], r["L"], r["num_layers"], r["output_size"], r["cus"], r["with_loss"])
        want = None if r["refused"] else (r["name"], r["shape"])
        if got != want:
            bad.append((r, got))
    assert not bad, "%d of %d rows differ, first: %r" % (len(bad), len(table), bad[0])


def test_anchors(monkeypatch):
    p = lambda B, env="", **kw: plan(monkeypatch, B, env, **kw)
    name = lambda *a, **kw: p(*a, **kw)[0]
    S, NB = 0, 4
    r = p(1280)
    assert r[0] == "k_serve6<4, 3, 2, 5, true>" and r[1][S] == 1 and r[1][NB] == 16, r
    r = p(1280, "PAIR=0")
    assert r[0] == "k_serve6<4, 3, 2, 10>" and r[1][NB] == 8, r
    r = p(64)
    assert r[0] == "k_serve6<4, 3, 2, 1>" and r[1][NB] == 4, r
    r = p(1024)
    assert r[0] == "k_serve6<4, 3, 4, 4>" and r[1][S] == 2, r
    r = p(2048)
    assert r[0] == "k_serve6<2, 3, 8, 4>" and r[1][S] == 4, r
    r = p(2049)
    assert r[0] == ROUNDS and r[1][NB] == 26, r
    assert p(2049, with_loss=1) is None
    assert p(2048, with_loss=1) is not None
    assert name(19213, "ROUNDS=0") == "k_serve5<4, 3, 2, 2>"
    assert name(19213, "PAIR=0") == "k_serve5<4, 3, 2, 2>"
    r = p(1281, "MAX_NB=20")
    assert r[0] == ROUNDS and r[1][NB] == 17, r
    assert name(1280, "SPLIT=3 RT=4") == "k_serve6<2, 3, 7, 4>"
    assert name(1280, "SPLIT=5 RT=2") == "k_serve6<2, 3, 11, 2>"
    assert name(1280, "SPLIT=3 RT=2") == "k_serve6<2, 3, 11, 2>"
    assert name(1285, "SPLIT=1 RT=10", L=2048) == "k_serve5<4, 3, 2, 2>"   # no form that wide
    r = p(1280, L=384)
    assert r[0] == "k_serve6<2, 3, 4, 4>" and r[1][S] == 3, r
    assert name(19213, L=768) == ROUNDS
    assert name(19213, L=512) == "k_serve5<4, 3, 2, 2>"
    assert name(1280, num_layers=0) == "k_serve<2, 3, 4>"
    assert name(1280, output_size=42).startswith("k_serve6<")   # 42 outputs: NDT 3
    assert name(1280, output_size=32) == "k_serve5<4, 2, 2, 2>"
    r = p(1280, cus=64)
    assert r[0] == "k_serve6<2, 3, 8, 4>" and r[1][S] == 1, r
    r = p(19213, "SERVE6=2")
    assert r[0] == "k_serve6<2, 3, 8, 4>" and r[1][S] == 4 and r[1][NB] == 301, r


def test_loss_is_refused_beyond_its_partials_buffer(monkeypatch):
    """The fused MSE writes one partial per 16 x 16 output tile into a buffer of P3D_SERVE6_ROWS / 16
    * 4 = 1024 words: ceil(B / 16) * 3 tiles fit up to B = 5456, whatever the knobs let through."""
    assert plan(monkeypatch, 5456, "SERVE6=2", with_loss=1) is not None
    assert plan(monkeypatch, 5457, "SERVE6=2", with_loss=1) is None
    assert b"p3d_serve_mse" in _p3d.lib().p3d_last_error()
    assert plan(monkeypatch, 5457, "MAX_NB=100", with_loss=1) is None
    assert plan(monkeypatch, 5457, "SERVE6=2") is not None   # without the loss the launch stands


def test_shapes_p3d_serve_refuses(monkeypatch):
    assert plan(monkeypatch, 0) is None
    assert plan(monkeypatch, 64, L=192) is None            # linear_size % 128
    assert plan(monkeypatch, 64, output_size=80) is None   # more than 64 outputs
    assert plan(monkeypatch, 64, num_layers=8) is None     # more than 7 blocks


def test_every_planned_form_is_in_the_built_library(monkeypatch, table):
    """The planner's list of forms and the instantiations in the code object are the same set: every
    kernel named over the table's inputs has a symbol (rocprof prints k_serve6's single-unit forms
    with their trailing pair flag: ", false>")."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not all(os.path.exists(os.path.join(llvm, t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not present")
    sys.path.insert(0, ROOT)
    from tools.kernel_resources import kernel_resources
    built = set(kernel_resources(_p3d.LIB_PATH))
    names = set()
    for r in table:
        got = plan(monkeypatch, r["B"], r["env"], r["L"], r["num_layers"], r["output_size"], r["cus"], r["with_loss"])
        if got:
            names.add(got[0])
    assert len(names) >= 15, names
    for n in sorted(names):
        sym = n[:-1] + ", false>" if n.startswith("k_serve6<") and not n.endswith("true>") else n
        assert "void %s(ServeArgs)" % sym in built, (n, sorted(k for k in built if "k_serve" in k))
