"""Dev tool: device times of the bones filter (the bones kind of csrc/p3d_vae.h, csrc/p3d_bones.h), one
JSON line per measurement, also appended to profiles/vae_bones_probe.jsonl.

At batch 64, alternated round by round, device events around `reps` back-to-back calls, medians
reported:

  (a) the 1376-input bones training step with its conversion launch: p3d_bones_from_joints
      (float32 form) of a [64, 48] pose, then train_step_device([x2d | bones | (feature table, idx)]);
  (b) the same step without the conversion launch (the bones segment already formed);
  (c) the 1360-input joint step [x2d | out_3d | (feature table, idx)], its counterpart of the
      parent commit, on the same box;

and (d) the bones forward alone at 2^20 rows against the HBM bound rows * 4 * in bytes, (e) both
conversion kernels at 2^20 rows as GB/s against the bytes they must move (192 in + 256 out a row;
256 in + 384 out a row).

    python tools/vae_bones_probe.py [--rounds 5] [--reps 200]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-pose-baseline_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from top_vae_3d_pose import bones, models  # noqa: E402

HBM_PEAK = 8.0e12        # bytes / s (MI355X)
F_BONES = (10.0, 100.0, 1.0, 100.0)
F_JOINT = (100.0, 0.02, 1.0)
ENC, LAT, DEC = (40, 32), 24, (32, 40)


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
    rounds, reps = arg("--rounds", 5), arg("--reps", 200)
    assert torch.cuda.is_available(), "the probe needs a GPU"
    out = []
    rng = np.random.default_rng(1)
    dev = torch.device("cuda")
    B = 64
    vb_ = models.VAEBones(1376, LAT, ENC, DEC, max_batch=B, seed=3)
    vb2 = models.VAEBones(1376, LAT, ENC, DEC, max_batch=B, seed=3)
    vj = models.VAE(1360, LAT, ENC, DEC, max_batch=B, seed=3)
    x2 = torch.from_numpy(rng.standard_normal((B, 32)).astype(np.float32)).to(dev)
    x3 = torch.from_numpy(rng.standard_normal((B, 48)).astype(np.float32)).to(dev)
    table = torch.from_numpy((0.1 * rng.standard_normal((100000, 1280))).astype(np.float32)).to(dev)   # 512 MB
    idx = torch.from_numpy(rng.permutation(100000)[:B].astype(np.int64)).to(dev)
    tj = torch.from_numpy(rng.standard_normal((B, 48)).astype(np.float32)).to(dev)
    tb = bones.convert_to_bones(tj)
    b64 = torch.empty((B, 64), dtype=torch.float32, device=dev)
    bones.convert_to_bones(x3, precise=False, out=b64)

    def step_with_conversion():
        bones.convert_to_bones(x3, precise=False, out=b64)
        vb_.train_step_device([x2, b64, (table, idx)], tb, F_BONES, 1e-4)

    cases = {"a_bones_step_with_conversion": step_with_conversion,
             "b_bones_step_without_conversion": lambda: vb2.train_step_device([x2, b64, (table, idx)], tb, F_BONES, 1e-4),
             "c_joint_1360_step": lambda: vj.train_step_device([x2, x3, (table, idx)], tj, F_JOINT, 1e-4)}
    for fn in cases.values():
        timed(fn, 20)                                # warm every shape
    us = {k: [] for k in cases}
    for _ in range(rounds):                          # alternate the cases round by round
        for k, fn in cases.items():
            us[k].append(round(timed(fn, reps), 3))
    rec = {"what": "vae_bones_step_b64", "shape": "1376-40-32-{24,24}-32-40-16-{16,48}", "reps": reps, "rounds": rounds}
    for k, v in us.items():
        rec[k + "_us"] = v
        rec[k + "_us_median"] = float(np.median(v))
    out.append(rec)
    for m in (vb_, vb2, vj):
        m.close()
    del table
    n = 1 << 20
    big = models.VAEBones(1376, LAT, ENC, DEC, max_batch=n, seed=3)
    xb = torch.randn((n, 1376), device=dev)
    eb = torch.randn((n, 24), device=dev)
    fwd = lambda: big.forward_device(xb, eps=eb)   # noqa: E731
    timed(fwd, 3)
    v = [round(timed(fwd, 10), 1) for _ in range(rounds)]
    med = float(np.median(v))
    nbytes = n * 4 * 1376
    out.append({"what": "vae_bones_fwd_2^20", "us": v, "us_median": med, "bytes_x": nbytes,
                "hbm_bound_us": round(1e6 * nbytes / HBM_PEAK, 1), "GBps": round(nbytes / med / 1e3, 1),
                "share_of_hbm_bound": round(1e6 * nbytes / HBM_PEAK / med, 3)})
    big.close()
    del xb, eb
    j = torch.randn((n, 48), device=dev)
    o = torch.empty((n, 64), device=dev)
    for name, fn, nbytes in (
            ("bones_from_joints_precise_2^20", lambda: bones.convert_to_bones(j, precise=True, out=o), n * (192 + 256)),
            ("bones_from_joints_float32_2^20", lambda: bones.convert_to_bones(j, precise=False, out=o), n * (192 + 256)),
            ("bones_to_joints_2^20", lambda: bones.convert_to_joints(o), n * (256 + 384))):
        timed(fn, 3)
        v = [round(timed(fn, 20), 1) for _ in range(rounds)]
        med = float(np.median(v))
        out.append({"what": name, "us": v, "us_median": med, "bytes": nbytes, "GBps": round(nbytes / med / 1e3, 1),
                    "share_of_hbm_peak": round(1e6 * nbytes / HBM_PEAK / med, 3),
                    "note": "bones_to_joints allocates its [2^20, 48] float64 result inside the timed call"
                    if "to_joints" in name else ""})
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "vae_bones_probe.jsonl"), "a") as f:
        for rec in out:
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
