"""The refusals of p3d_vae_seq_filter / p3d_vae_seq_filter_mc BEHIND a live filter handle: the two
calls share one checked fill of VaeSeqArgs (vae_seq_args, csrc/p3d_vae_host.h), and the order of
its checks and the words of every message are the ones the calls had when each wrote them out.
tests/golden/lift_errors_handle_parent.json holds (return code, p3d_last_error) of
tests/lift_error_cases.handle_cases from that library (tools/record_lift_errors.py --gpu).  Every
call is refused before a launch; its pointers are real device memory all the same."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "lift_errors_handle_parent.json")

import lift_error_cases  # noqa: E402


def handle_rows():
    """handle_cases against the library _p3d loads, with filters and memory of its own."""
    import torch
    import _p3d
    from top_vae_3d_pose import models
    flt = {"seq": models.VAE(144, 24, [40, 32], [32, 40], max_batch=64, seed=3),
           "flat": models.VAE(104, 24, [40, 32], [32, 40], max_batch=64, seed=3),
           "bones": models.VAEBones(64, 8, (24,), (24,), max_batch=64, seed=1)}
    mem = torch.zeros((20 * 16384 + 256,), dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 9, 30], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rows = lift_error_cases.run_handles(_p3d.lib(), {k: m._h for k, m in flt.items()},
                                        (mem.data_ptr() + 255) // 256 * 256, off.data_ptr())
    torch.cuda.synchronize()
    for m in flt.values():
        m.close()
    return rows


@pytest.mark.gpu
def test_refusals_behind_a_live_filter_are_the_parents():
    import _p3d
    with open(GOLD) as f:
        want = json.load(f)
    got = handle_rows()
    assert len(want) >= 30 and all(r["rc"] == _p3d.P3D_ERR_ARG for r in want)
    assert [r["id"] for r in got] == [r["id"] for r in want]
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, "%d of %d calls answer differently, first: want %r, got %r" % (len(bad), len(want), *bad[0])
    by = {r["id"]: r["msg"] for r in want}
    assert by["vae_seq_filter/bones_bad_S"].endswith("a bones filter has no sequence form")
    assert by["vae_seq_filter_mc/bones_bad_S"].endswith("direction cosines do not average")
    assert by["vae_seq_filter/misaligned_fstate"].endswith("pred, eps, target, state and ref must be 16-byte aligned")
    assert by["vae_seq_filter_mc/misaligned_ref_var"].endswith("state, ref and ref_var must be 16-byte aligned")
