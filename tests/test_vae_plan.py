"""The VAE filter's planner (csrc/p3d_vae_layout.h) and the handle built on it (csrc/p3d_vae_host.h).

  * The library answers what the build before the planner moved answered, through the ABI alone
    (tests/golden/vae_plan_parent.json, recorded from that build): the *_lds_bytes calls and
    p3d_vae_cat_check here, what a created filter reports on the GPU.
  * The planner alone -- tests/host/vae_plan_main.cpp includes nothing but the planner's header -- is
    built by the host compiler with AddressSanitizer and UBSan, run as a child process over the same
    shapes, and its sizes equal the library's.
  * Two filters of different size alive in one process: the larger runs the same after the smaller
    was created (the dynamic-LDS attribute is the process's, not a filter's).
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import _p3d
import vae_plan_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    with open(pc.GOLDEN) as f:
        return json.load(f)


def test_golden_covers_the_cases(golden):
    assert list(golden["shapes"]) == [n for n, _, _ in pc.cases()]
    for name, kind, shape in pc.cases():
        rec = golden["shapes"][name]
        assert (rec["kind"], json.loads(json.dumps(shape))) == (kind, rec["shape"]), name
    deepest = golden["shapes"]["bones_deepest"]["gpu"]
    assert len(deepest["params"]) == 26                      # the descriptor's tensor bound


def test_lds_answers_equal_the_parent(golden):
    lib = _p3d.lib()
    for name, _, shape in pc.cases():
        assert pc.host_answers(lib, shape) == golden["shapes"][name]["host"], name


def test_cat_check_answers_equal_the_parent(golden):
    assert len(golden["cat"]) == len(pc.CAT_CASES) + 1
    assert pc.cat_answers(_p3d.lib()) == golden["cat"]


def _host_compiler():
    for cxx in ("g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    return None


def test_planner_alone_under_sanitizers(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "vae_plan_main")
    # the sanitizers' runtimes linked statically where the compiler has them that way (g++ needs the flags,
    # clang does it by default), so that the program needs nothing preloaded; else as the compiler links them
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
           "-o", exe, os.path.join(HERE, "host", "vae_plan_main.cpp")]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    cases = pc.cases()
    text = "".join("%d %d %d %s %d %d %s %d\n" % (kind, s[0], len(s[1]), " ".join(map(str, s[1])), s[2], len(s[3]),
                                                   " ".join(map(str, s[3])), s[4]) for _, kind, s in cases)
    run = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases)
    lib = _p3d.lib()
    for (name, kind, shape), line in zip(cases, lines):
        v = [int(x) for x in line.split()]
        assert len(v) == 19, (name, line)
        status, lds, other_lds, dec_lds, dec_staggered, seq_lds = v[:6]
        host = pc.host_answers(lib, shape)
        own, other = ("bones_lds", "lds") if kind else ("lds", "bones_lds")
        if status < 0:                                        # vae_check_shape refuses: the library answers 0
            assert host[own] == 0 and host[other] == 0, name
            continue
        assert (lds, other_lds) == (host[own], host[other]), name
        assert dec_staggered == host["dec_lds"][kind], name
        if not kind:
            assert host["seq_lds"] == [seq_lds, seq_lds], name
        assert (status == 0) == (lds <= 163840 and name != "dup_width"), name
        if status == 0:
            assert 0 < dec_lds <= lds, name
            nl, nt = v[9], v[10]
            assert nl <= 11 and nt <= 26 and v[18] == v[6], name       # the arrays' bounds; one index per parameter
    deepest = [int(x) for x in lines[[n for n, _, _ in cases].index("bones_deepest")].split()]
    assert (deepest[9], deepest[10]) == (11, 26)


@pytest.mark.gpu
def test_created_filters_report_what_the_parent_did(golden):
    """Every shape created once at max_batch 64 and 200, nothing launched: the parameter table, the
    flat buffers' sizes, p3d_vae_workspace, p3d_vae_kind, and the create error of the refused ones."""
    lib = _p3d.lib()
    refused = 0
    for name, kind, shape in pc.cases():
        got = pc.gpu_answers(lib, kind, shape)
        assert json.loads(json.dumps(got)) == golden["shapes"][name]["gpu"], name
        refused += "error" in got
    assert refused == 4                      # VAE_REFUSED, the two refused golden shapes, the duplicate width


@pytest.mark.gpu
def test_a_filter_runs_the_same_after_a_smaller_one_is_created():
    """The large filter's forward, loss, decode and sequence filter at B = 17 (one full tile and one
    row), then the same four on a small filter created afterwards, then the large one's again: the
    same bits as the first time."""
    import torch
    from top_vae_3d_pose import models
    large, small = (144, (40, 32), 24, (32, 40), 48), (48, (8,), 8, (24,), 48)
    assert pc.host_answers(_p3d.lib(), large)["lds"] == 161664 > pc.host_answers(_p3d.lib(), small)["lds"]
    B, factors, off = 17, (100.0, 0.02, 1.0), [0, 5, 8]

    def make(shape, seed):
        m = models.VAE(shape[0], shape[2], shape[1], shape[3], shape[4], max_batch=64, seed=seed)
        m.initialize(seed)
        g = torch.Generator().manual_seed(seed)
        data = {k: torch.randn((n, w), generator=g).cuda() for k, n, w in
                (("x", B, shape[0]), ("t", B, 48), ("eps", B, shape[2]), ("z", B, shape[2]), ("pred", off[-1], 48),
                 ("eps_seq", off[-1], shape[2]))}
        return m, data

    def four(m, d):
        out = [m.forward_device(d["x"], eps=d["eps"])["y"], m.loss_device(d["x"], d["t"], factors, eps=d["eps"]),
               m.decode(d["z"]), m.filter_sequences(d["pred"], off, eps=d["eps_seq"], ctr=0)["ref"]]
        out = [o.cpu().numpy().copy() for o in out]
        assert all(np.isfinite(o).all() for o in out)
        return out

    m_large, d_large = make(large, 3)
    try:
        first = four(m_large, d_large)
        m_small, d_small = make(small, 4)
        try:
            four(m_small, d_small)
            again = four(m_large, d_large)
        finally:
            m_small.close()
    finally:
        m_large.close()
    for a, b in zip(first, again):
        assert a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))
