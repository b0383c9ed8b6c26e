"""Dev tool: device times of the decoder on its own (csrc/p3d_vae_dec.h) beside the forward launch
over the same rows, one JSON line per measurement, also appended to profiles/vae_dec_probe.jsonl.

On the default filter, in one process, device events around `reps` back-to-back calls, the cases
alternated over `rounds` rounds (at least 5), every round's figure and the median reported:

  * p3d_vae_decode with z given, p3d_vae_decode with z drawn (the prior stream) and
    p3d_vae_forward (caller's eps, y alone) at 2^20 rows -- each decode at every grid the
    CU's LDS allows (p3d_vae_dec_set_grid: 1 .. workgroups per CU), the default marked;
  * the same three at 64 rows (one workgroup): the launch cost.

    python tools/vae_dec_probe.py [--rounds 5] [--reps 10]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-pose-baseline_amd"))
sys.path.insert(0, ROOT)

import ctypes  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _p3d  # noqa: E402
from top_vae_3d_pose import models  # noqa: E402

LDS_LIMIT = 163840


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps      # microseconds per call


def main():
    arg = lambda k, d: int(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d   # noqa: E731
    rounds, reps = max(arg("--rounds", 5), 5), arg("--reps", 10)
    lib, st = _p3d.lib(), _p3d.stream_handle
    m = models.VAE(48, 24, [40, 32], [32, 40], max_batch=64, seed=3)
    dec = (ctypes.c_int32 * 2)(32, 40)
    enc = (ctypes.c_int32 * 2)(40, 32)
    dec_lds = int(lib.p3d_vae_dec_lds_bytes(24, 2, dec, 48, 0))
    fwd_lds = int(lib.p3d_vae_lds_bytes(48, 2, enc, 24, 2, dec, 48))
    fit = LDS_LIMIT // dec_lds
    default = min(4, fit)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = []
    for n, r in ((1 << 20, reps), (64, 20 * reps)):
        x = torch.randn((n, 48), device="cuda")
        e = torch.randn((n, 24), device="cuda")
        z = torch.randn((n, 24), device="cuda")
        y = torch.empty((n, 48), device="cuda")

        def fwd():
            _p3d.check(lib.p3d_vae_forward(m._h, _p3d.ptr(x), n, _p3d.ptr(e), 1, _p3d.ptr(y), None, None, None, None,
                                           None, st()), "p3d_vae_forward")

        def dec_given():
            _p3d.check(lib.p3d_vae_decode(m._h, _p3d.ptr(z), n, 0, 0, _p3d.ptr(y), None, st()), "p3d_vae_decode")

        def dec_drawn():
            _p3d.check(lib.p3d_vae_decode(m._h, None, n, 1, 0, _p3d.ptr(y), None, st()), "p3d_vae_decode")

        def at(grid, fn):
            def run():
                m.set_dec_grid(grid)
                return timed(fn, r)
            return run

        grids = range(1, fit + 1) if n > 64 else (default,)     # (at 64 rows the launch is one workgroup)
        cases = {"forward": lambda: timed(fwd, r)}
        for g in grids:
            cases["decode_z_given_wgs%d" % g] = at(g, dec_given)
            cases["decode_z_drawn_wgs%d" % g] = at(g, dec_drawn)
        for fn in cases.values():
            fn()                                                # warm
        us = {k: [] for k in cases}
        for _ in range(rounds):                                 # alternate the cases round by round
            for k, fn in cases.items():
                us[k].append(round(fn(), 2))
        m.set_dec_grid(0)
        rec = {"what": "vae_dec_probe", "rows": n, "reps": r, "rounds": rounds, "cus": cus, "dec_lds_bytes": dec_lds,
               "fwd_lds_bytes": fwd_lds, "default_wgs_per_cu": default,
               "bytes_decode_z_given": n * 4 * (24 + 48), "bytes_decode_z_drawn": n * 4 * 48,
               "bytes_forward": n * 4 * (48 + 24 + 48)}
        for k, v in us.items():
            rec[k + "_us"] = v
            rec[k + "_us_median"] = float(np.median(v))
            rec[k + "_us_range"] = [min(v), max(v)]
        out.append(rec)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "vae_dec_probe.jsonl"), "a") as f:
        for rec in out:
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
    m.close()


if __name__ == "__main__":
    main()
