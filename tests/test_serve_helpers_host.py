"""The rounds form with helper waves, without a GPU: what the planner names for a long launch under
P3D_SERVE6_HELPERS, and the helper kernel's resources in the built code object (tools/kernel_resources.py
reads the metadata note and nothing else)."""
import ctypes
import json
import os
import sys

import pytest

import _p3d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "serve_plan_parent.json")
KNOBS = ("P3D_SERVE6", "P3D_SERVE6_MAX_NB", "P3D_SERVE6_SPLIT", "P3D_SERVE6_RT", "P3D_SERVE6_DEPTH",
         "P3D_SERVE6_PAIR", "P3D_SERVE6_ROUNDS", "P3D_SERVE6_HELPERS")
HELPERS = "k_serve6_rounds<4, 3, 2, 5>"
PARENT = "k_serve6_rounds_w4<4, 3, 2, 5>"
LLVM = "/opt/rocm/lib/llvm/bin"


def plan(monkeypatch, B, env="", L=1024, num_layers=2, output_size=48, cus=256, with_loss=0):
    """The kernel name of the launch, or None where it is refused with P3D_ERR_ARG."""
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
    return name.value.decode()


def _built():
    if not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not present")
    sys.path.insert(0, ROOT)
    from tools.kernel_resources import kernel_resources
    return kernel_resources(_p3d.LIB_PATH)


@pytest.mark.parametrize("L", [768, 1024])
def test_long_launch_names(monkeypatch, L):
    p = lambda env="": plan(monkeypatch, 19213, env, L=L)   # noqa: E731
    assert p() == HELPERS
    assert p("HELPERS=1") == HELPERS
    assert p("HELPERS=0") == PARENT
    assert p("ROUNDS=0") == "k_serve5<4, 3, 2, 2>"
    assert p("PAIR=0") == "k_serve5<4, 3, 2, 2>"
    assert p("ROUNDS=0 HELPERS=0") == "k_serve5<4, 3, 2, 2>"
    assert p("PAIR=0 HELPERS=0") == "k_serve5<4, 3, 2, 2>"


def test_the_knob_touches_long_launches_only(monkeypatch):
    """The 20-step launch, a lone request and a forced k_serve6 plan are what they were."""
    for B, env in ((1280, ""), (64, ""), (2048, ""), (1280, "PAIR=0")):
        assert plan(monkeypatch, B, env) == plan(monkeypatch, B, (env + " HELPERS=0").strip()), (B, env)
    assert plan(monkeypatch, 1280, "HELPERS=0") == "k_serve6<4, 3, 2, 5, true>"
    assert plan(monkeypatch, 1281, "MAX_NB=20 HELPERS=0") == PARENT
    assert plan(monkeypatch, 2049, "HELPERS=0", with_loss=1) is None


def test_every_name_under_either_knob_value_is_built(monkeypatch):
    built = set(_built())
    with open(GOLD) as f:
        table = json.load(f)
    names = set()
    for r in table:
        for extra in ("", " HELPERS=0"):
            got = plan(monkeypatch, r["B"], (r["env"] + extra).strip(), r["L"], r["num_layers"], r["output_size"],
                       r["cus"], r["with_loss"])
            if got:
                names.add(got)
    assert HELPERS in names and PARENT in names, names
    for n in sorted(names):
        sym = n[:-1] + ", false>" if n.startswith("k_serve6<") and not n.endswith("true>") else n
        assert "void %s(ServeArgs)" % sym in built, (n, sorted(k for k in built if "k_serve" in k))


def test_helper_kernel_resources():
    """Eight waves, two per SIMD, one register allocation for both roles: 256 registers (vgpr_count is
    the wave's whole allocation, accumulation registers included), nothing spilled, no scratch, no
    dynamic stack, and LDS within the CU's 160 KB."""
    res = _built()
    r = res["void %s(ServeArgs)" % HELPERS]
    assert r.get("private_segment_fixed_size", 0) == 0, r
    assert r.get("vgpr_spill_count", 0) == 0, r
    assert max(r.get("vgpr_count", 0), r.get("agpr_count", 0)) <= 256, r
    assert r.get("vgpr_count", 0) >= r.get("agpr_count", 0), r   # (the total, not the arch VGPRs alone)
    assert r.get("group_segment_fixed_size", 0) <= 160 * 1024, r
    assert not r.get("uses_dynamic_stack", False), r


def test_parent_kernel_uses_no_scratch():
    res = _built()
    r = res["void %s(ServeArgs)" % PARENT]
    assert r.get("private_segment_fixed_size", 0) == 0, r
    assert r.get("vgpr_spill_count", 0) == 0, r
    assert not r.get("uses_dynamic_stack", False), r
