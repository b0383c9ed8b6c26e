"""Dev tool: device times of sample()'s numbers (csrc/p3d_sample.h, predict_3dpose.sample_rows)
beside the composition of existing calls they replace, one JSON line per measurement, also appended
to profiles/sample_probe.jsonl.

In one process, device events around `reps` back-to-back calls, the cases alternated over `rounds`
rounds (at least 5), every round's figure and the median reported:

  (a) p3d_sample_world at 2^20 rows (U = 48 float32 input, one camera), with and without root,
      against the composed calls over the same rows: p3d_unnormalize, the root add (torch),
      p3d_cam_transform(inverse = 1), p3d_root_center; and the fused launch with four cameras
      mixed row by row.  Bytes are what each form must move, computed from the shapes;
  (b) sample()'s device work at the H3.6M test split's size (240 sequences, 524,599 frames,
      synthetic rows, 8 cameras; the reference's 2 x 1024 model): predict_3dpose.sample_rows --
      one forward sweep, one launch per tensor -- against the same work one sequence at a time
      (forward, p3d_unnormalize x 3, root add, p3d_cam_transform x 2, p3d_root_center x 2 per
      sequence).

    python tools/sample_probe.py [--rounds 5] [--reps 10]
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-pose-baseline_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import data_pipeline as dp  # noqa: E402
import data_utils  # noqa: E402
import linear_model  # noqa: E402
import predict_3dpose  # noqa: E402
from synth_cameras import synth_cameras  # noqa: E402

H36M_TEST_SEQUENCES, H36M_TEST_FRAMES = 240, 524599


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps      # microseconds per call


def run_cases(cases, rounds, reps):
    for fn in cases.values():
        fn()                                     # warm
    torch.cuda.synchronize()
    us = {k: [] for k in cases}
    for _ in range(rounds):                      # alternate the cases round by round
        for k, fn in cases.items():
            us[k].append(round(timed(fn, reps), 2))
    return us


def report(rec, us, nbytes):
    for k, v in us.items():
        med = float(np.median(v))
        rec[k + "_us"] = v
        rec[k + "_us_median"] = med
        rec[k + "_us_range"] = [min(v), max(v)]
        if k in nbytes:
            rec[k + "_bytes"] = nbytes[k]
            rec[k + "_TBps"] = round(nbytes[k] / med * 1e-6, 3)
    return rec


def stats3(rng):
    use3, _ = data_utils.dimension_sets(3)
    mean, std = np.zeros(96), np.zeros(96)
    mean[use3] = rng.uniform(-500, 500, len(use3))
    std[use3] = rng.uniform(50, 300, len(use3))
    return dp.as_device(mean), dp.as_device(std), dp.as_device(np.asarray(use3, np.int32), torch.int32)


def composed(yn, mean, std, use, cam, root, scratch):
    """The existing calls over the same rows (one camera): the per-sequence form of sample()."""
    x = dp.unnormalize(yn, mean, std, use, 96, out=scratch)
    if root is not None:
        x = x + root.repeat(1, 32)
    w = dp.camera_to_world(x.view(-1, 3), cam)[0].view(-1, 96)
    return dp.root_center(w)[0]


def part_a(rounds, reps):
    n, U = 1 << 20, 48
    rng = np.random.default_rng(1)
    mean, std, use = stats3(rng)
    _, packed, _ = synth_cameras(rng, subjects=(9,))
    cams = dp.as_device(packed[0])
    yn = torch.randn((n, U), dtype=torch.float32, device="cuda")
    root = torch.randn((n, 3), dtype=torch.float64, device="cuda") * 1000.0
    cor = torch.randint(0, 4, (n,), dtype=torch.int32, device="cuda")
    out = torch.empty((n, 96), dtype=torch.float64, device="cuda")
    scratch = torch.empty((n, 96), dtype=torch.float64, device="cuda")
    cases = {
        "fused_root": lambda: dp.sample_world(yn, mean, std, use, cams[:1], None, root, out=out),
        "fused_no_root": lambda: dp.sample_world(yn, mean, std, use, cams[:1], None, None, out=out),
        "fused_root_mixed_cams": lambda: dp.sample_world(yn, mean, std, use, cams, cor, root, out=out),
        "composed_root": lambda: composed(yn, mean, std, use, cams[:1], root, scratch),
        "composed_no_root": lambda: composed(yn, mean, std, use, cams[:1], None, scratch),
    }
    row = 96 * 8
    nbytes = {
        "fused_root": n * (4 * U + 24 + row),
        "fused_no_root": n * (4 * U + row),
        "fused_root_mixed_cams": n * (4 * U + 24 + 4 + row),
        # unnormalize (U in, row out); root tiled (24 in, row out) and added (2 rows in, row out);
        # transform (row in, row out); root_center (row in, row + 24 out)
        "composed_root": n * ((4 * U + row) + (24 + row) + 3 * row + 2 * row + (2 * row + 24)),
        "composed_no_root": n * ((4 * U + row) + 2 * row + (2 * row + 24)),
    }
    same = torch.equal(dp.sample_world(yn, mean, std, use, cams[:1], None, root).view(torch.int64),
                       composed(yn, mean, std, use, cams[:1], root, scratch).view(torch.int64))
    rec = {"what": "sample_probe_a", "rows": n, "U": U, "reps": reps, "rounds": rounds,
           "cus": torch.cuda.get_device_properties(0).multi_processor_count, "fused_equals_composed": bool(same)}
    return report(rec, run_cases(cases, rounds, reps), nbytes)


def part_b(rounds, reps):
    S, N = H36M_TEST_SEQUENCES, H36M_TEST_FRAMES
    rng = np.random.default_rng(2)
    cuts = np.sort(rng.choice(np.arange(1, N), size=S - 1, replace=False))
    off = np.concatenate([[0], cuts, [N]]).astype(np.int64)
    lens = np.diff(off)
    _, packed, _ = synth_cameras(rng, subjects=(9, 11))
    cam_table = packed.reshape(-1, 21)                                     # 8 cameras
    cam_of_seq = rng.integers(0, len(cam_table), S)
    use2, _ = data_utils.dimension_sets(2)
    use3, _ = data_utils.dimension_sets(3)
    mean3, std3, _ = stats3(rng)
    stats = {"data_mean_2d": dp.as_device(rng.uniform(200, 800, 64)), "data_std_2d": dp.as_device(rng.uniform(20, 120, 64)),
             "dim_to_use_2d": dp.as_device(np.asarray(use2, np.int32), torch.int32), "data_mean_3d": mean3,
             "data_std_3d": std3, "dim_to_use_3d": dp.as_device(np.asarray(use3, np.int32), torch.int32)}
    model = linear_model.LinearModel(1024, 2, True, True, True, 128, 1e-3, tempfile.mkdtemp(prefix="p3d_probe_"),
                                     seed=3, max_batch=8192)
    X = torch.randn((N, 32), dtype=torch.float32, device="cuda")
    Y = torch.randn((N, 48), dtype=torch.float32, device="cuda")
    root = torch.randn((N, 3), dtype=torch.float64, device="cuda") * 1000.0
    cams = dp.as_device(cam_table)
    cam_of_row = torch.repeat_interleave(dp.as_device(cam_of_seq.astype(np.int32), torch.int32),
                                         dp.as_device(lens, torch.int64), output_size=N)
    world = (cams, cam_of_row, root)
    scratch = torch.empty((int(lens.max()), 96), dtype=torch.float64, device="cuda")
    P = torch.empty((N, 48), dtype=torch.float32, device="cuda")

    def fused():
        return predict_3dpose.sample_rows(model, X, Y, stats, world)

    def per_sequence():
        last = None
        for i in range(S):
            lo, hi = int(off[i]), int(off[i + 1])
            for s in range(lo, hi, model.max_batch):
                e = min(hi, s + model.max_batch)
                model.forward_device(X[s:e], False, 1.0, out=P[s:e])
            cam = cams[int(cam_of_seq[i]):int(cam_of_seq[i]) + 1]
            enc = dp.unnormalize(X[lo:hi], stats["data_mean_2d"], stats["data_std_2d"], stats["dim_to_use_2d"], 64)
            dec = composed(Y[lo:hi], mean3, std3, stats["dim_to_use_3d"], cam, root[lo:hi], scratch[:hi - lo])
            pose = composed(P[lo:hi], mean3, std3, stats["dim_to_use_3d"], cam, None, scratch[:hi - lo])
            last = (enc, dec, pose)
        return last

    f, p = fused(), per_sequence()
    lo = int(off[-2])
    same = [torch.equal(a[lo:].contiguous().view(torch.int64), b.contiguous().view(torch.int64)) for a, b in zip(f, p)]
    del f, p
    us = run_cases({"sample_rows": fused, "per_sequence": per_sequence}, rounds, reps)
    rec = {"what": "sample_probe_b", "sequences": S, "rows": N, "cameras": int(len(cam_table)), "reps": reps,
           "rounds": rounds, "model": "1024x2 residual batch_norm max_norm, max_batch 8192",
           "last_sequence_enc_in_equal": same[0], "last_sequence_dec_out_equal": same[1],
           "last_sequence_poses3d_equal": same[2]}
    rec = report(rec, us, {})
    model.close()
    return rec


def main():
    arg = lambda k, d: int(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d   # noqa: E731
    rounds, reps = max(arg("--rounds", 5), 5), arg("--reps", 10)
    if not torch.cuda.is_available():
        raise SystemExit("sample_probe: no GPU is visible (there is nothing to measure without one)")
    out = [part_a(rounds, reps), part_b(rounds, max(1, reps // 5))]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sample_probe.jsonl"), "a") as f:
        for rec in out:
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
