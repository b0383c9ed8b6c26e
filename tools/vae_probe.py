"""Dev tool: device times of the VAE filter (csrc/p3d_vae.h), one JSON line per measurement, also
appended to profiles/vae_probe.jsonl.

  * the B = 64 training step in its one-launch form and in the partials (two-launch) form, beside
    p3d_empty_launch on the same device (the launch floor) -- device events around `reps`
    back-to-back calls, the three alternated over `rounds` rounds, medians reported;
  * the lifter's evaluation forward (p3d_serve) + the step, per batch: what train_step_vae costs;
  * k_vae_fwd at 2^20 rows against its two bounds: the bytes it must move (x in, y out) over the
    HBM peak, and its FLOPs over the fp32 MFMA peak.

    python tools/vae_probe.py [--rounds 5] [--reps 200]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-pose-baseline_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _p3d  # noqa: E402
import linear_model  # noqa: E402
from top_vae_3d_pose import models  # noqa: E402

HBM_PEAK = 8.0e12        # bytes / s (MI355X)
F32_MFMA_PEAK = 157.3e12  # FLOP / s, v_mfma_f32_16x16x4_f32 (= the fp32 vector peak)
FACTORS = (100.0, 0.02, 1.0)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps      # microseconds per call


def flops_per_row(vae):
    return 2 * sum(int(np.prod(s)) for n, s, _ in vae.param_table if n.endswith("/kernel"))


def main():
    arg = lambda k, d: int(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d   # noqa: E731
    rounds, reps = arg("--rounds", 5), arg("--reps", 200)
    out = []
    rng = np.random.default_rng(1)
    lifter = linear_model.LinearModel(1024, 2, True, True, False, 64, 1e-3, "/tmp/p3d_vae_probe", seed=5)
    one = models.VAE(48, 24, [40, 32], [32, 40], max_batch=64, seed=3)
    two = models.VAE(48, 24, [40, 32], [32, 40], max_batch=64, seed=3)
    two.set_form(1)
    x2 = torch.from_numpy(rng.standard_normal((64, 32)).astype(np.float32)).cuda()
    x = torch.from_numpy(rng.standard_normal((64, 48)).astype(np.float32)).cuda()
    t = torch.from_numpy(rng.standard_normal((64, 48)).astype(np.float32)).cuda()
    y3 = torch.empty((64, 48), device="cuda")
    lib, st = _p3d.lib(), _p3d.stream_handle

    def empty():
        _p3d.check(lib.p3d_empty_launch(lifter._h, 1, st()), "p3d_empty_launch")

    def lifter_step():
        lifter.serve_device(x2, out=y3)
        one.train_step_device(y3, t, FACTORS, 1e-4)

    cases = {"empty_launch": empty,
             "step_one_launch": lambda: one.train_step_device(x, t, FACTORS, 1e-4),
             "step_two_launch": lambda: two.train_step_device(x, t, FACTORS, 1e-4),
             "lifter_plus_step": lifter_step}
    for fn in cases.values():
        timed(fn, 20)                                # warm every shape
    us = {k: [] for k in cases}
    for _ in range(rounds):                          # alternate the cases round by round
        for k, fn in cases.items():
            us[k].append(round(timed(fn, reps), 3))
    rec = {"what": "vae_step_b64", "reps": reps, "rounds": rounds}
    for k, v in us.items():
        rec[k + "_us"] = v
        rec[k + "_us_median"] = float(np.median(v))
    out.append(rec)
    lifter.check_errors()
    # the filter alone at 2^20 rows
    big = models.VAE(48, 24, [40, 32], [32, 40], max_batch=64, seed=3)
    n = 1 << 20
    xb = torch.randn((n, 48), device="cuda")
    eb = torch.randn((n, 24), device="cuda")
    yb = torch.empty((n, 48), device="cuda")

    def fwd(eps):
        _p3d.check(lib.p3d_vae_forward(big._h, _p3d.ptr(xb), n, _p3d.ptr(eps), 1, _p3d.ptr(yb), None, None, None, None,
                                       None, st()), "p3d_vae_forward")

    for tag, eps in (("caller_eps", eb), ("philox_eps", None)):
        timed(lambda: fwd(eps), 3)
        v = [round(timed(lambda: fwd(eps), 10), 1) for _ in range(rounds)]
        nbytes = n * 4 * (48 + 48 + (24 if eps is not None else 0))
        fl = n * flops_per_row(big)
        med = float(np.median(v))
        out.append({"what": "vae_fwd_2^20", "eps": tag, "us": v, "us_median": med, "bytes": nbytes, "flop": fl,
                    "hbm_bound_us": round(1e6 * nbytes / HBM_PEAK, 1), "mfma_bound_us": round(1e6 * fl / F32_MFMA_PEAK, 1),
                    "GBps": round(nbytes / med / 1e3, 1), "TFLOPs": round(fl / med / 1e6, 2),
                    "share_of_bound": round(max(nbytes / HBM_PEAK, fl / F32_MFMA_PEAK) * 1e6 / med, 3)})
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "vae_probe.jsonl"), "a") as f:
        for rec in out:
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
    for m in (one, two, big):
        m.close()
    lifter.close()


if __name__ == "__main__":
    main()
