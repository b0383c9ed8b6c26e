"""Dev tool: a whole OpenPose clip through ClipLifter.lift_clip (one p3d_clip_lift between pinned
rows) against a FrameLifter(batch=1) loop over the same frames -- the loop a user writes around
the per-frame API, with the smoothing and post-processing left out of it, so the loop's side is a
lower bound of that workflow -- in one process, alternating, at N in {9, 256, 4096}; then the
device time of p3d_clip_prepare and p3d_clip_finish (device events around back-to-back calls)
against the bytes they must move.  Prints one JSON line per measurement.

    python tools/clip_probe.py            # the A/B and the two calls' device times
    python tools/clip_probe.py --kernels  # only the two calls, few repetitions (for a kernel trace)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-pose-baseline_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _p3d  # noqa: E402
import data_pipeline as dp  # noqa: E402
import data_utils  # noqa: E402
import linear_model  # noqa: E402
import openpose_frontend as of  # noqa: E402


def clip(rng, n):
    xy = rng.uniform(100, 900, (n, 36))
    xy[rng.random((n, 36)) < 0.2] = 0.0          # dropped joints, as OpenPose leaves them
    return xy


def bytes_prepare(n, u2=32):
    """Bytes k_clip_in must move: xy in, xy_s and x out (the halo re-reads and the summaries left out)."""
    return n * (36 * 8 + 36 * 8 + u2 * 4)


def bytes_finish(n, u3=48):
    """Bytes k_clip_out must move: y and the two spine columns in, poses and src out."""
    return n * (u3 * 4 + 2 * 8 + 96 * 8 + 4)


def device_times(n, reps, rng):
    """Mean device microseconds of p3d_clip_prepare and p3d_clip_finish at n frames."""
    lib, p, st = _p3d.lib(), _p3d.ptr, _p3d.stream_handle
    use2, _ = data_utils.dimension_sets(2)
    use3, _ = data_utils.dimension_sets(3)
    xy = dp.as_device(clip(rng, n))
    m2, s2 = dp.as_device(rng.uniform(200, 600, 64)), dp.as_device(rng.uniform(50, 150, 64))
    m3, s3 = dp.as_device(rng.uniform(-400, 400, 96)), dp.as_device(rng.uniform(30, 300, 96))
    u2, u3 = dp._dims(use2, 64, "probe"), dp._dims(use3, 96, "probe")
    x = torch.empty((n, 32), dtype=torch.float32, device="cuda")
    y = torch.randn((n, 48), dtype=torch.float32, device="cuda")
    xy_s = torch.empty((n, 36), dtype=torch.float64, device="cuda")
    poses = torch.empty((n, 96), dtype=torch.float64, device="cuda")
    src = torch.empty((n,), dtype=torch.int32, device="cuda")
    nbytes = int(lib.p3d_clip_workspace(n))
    work = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device="cuda")

    def prep():
        _p3d.check(lib.p3d_clip_prepare(p(xy), n, 1, p(m2), p(s2), p(u2), 32, p(x), p(xy_s), p(work), nbytes, st()),
                   "p3d_clip_prepare")

    def fin():
        _p3d.check(lib.p3d_clip_finish(p(y), n, p(xy_s), p(m3), p(s3), p(u3), 48, 96, 1, p(poses), p(src), p(work),
                                       nbytes, st()), "p3d_clip_finish")

    out = {"what": "clip_calls_device_time", "N": n, "reps": reps}
    for name, fn, nb in (("prepare", prep, bytes_prepare(n)), ("finish", fin, bytes_finish(n))):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / reps
        out[name + "_us"] = round(us, 2)
        out[name + "_bytes"] = nb
        out[name + "_GBps"] = round(nb / us / 1e3, 1)
    return out


def main():
    kernels_only = "--kernels" in sys.argv
    rng = np.random.default_rng(900)
    if kernels_only:
        for n in (4096, 1 << 20):
            print(json.dumps(device_times(n, 20, rng)), flush=True)
        return
    m = linear_model.LinearModel(1024, 2, True, True, False, 64, 1e-3, "/tmp/p3d_clip_probe", seed=5, max_batch=8192)
    use2, _ = data_utils.dimension_sets(2)
    _, ign3 = data_utils.dimension_sets(3)
    stats = (rng.uniform(200, 600, 64), rng.uniform(50, 150, 64), use2, rng.uniform(-400, 400, 96),
             rng.uniform(30, 300, 96), ign3)
    fl = of.FrameLifter(m, *stats, batch=1)
    cl = of.ClipLifter(m, *stats, max_frames=4096)
    for n in (9, 256, 4096):
        xy = clip(rng, n)
        mapped = of.map_frames(xy)[:, None, :]           # the loop's frames, mapped once outside the clock
        reps_clip = max(20, 40000 // n)
        reps_loop = max(2, 8192 // n)
        out = {"what": "clip_vs_frame_loop", "N": n, "clip_fps": [], "loop_fps": [], "clip_us": [], "loop_us": []}
        for _ in range(3):                               # warm both shapes
            cl.lift_clip(xy)
            for e in mapped[:16]:
                fl.lift_mapped(e)
        for _ in range(3):                               # alternate: clip, loop, clip, loop, ...
            t0 = time.perf_counter()
            for _ in range(reps_clip):
                cl.lift_clip(xy)                         # (returns after its own stream synchronise)
            dt = (time.perf_counter() - t0) / reps_clip
            out["clip_us"].append(round(1e6 * dt, 1))
            out["clip_fps"].append(round(n / dt))
            t0 = time.perf_counter()
            for _ in range(reps_loop):
                for e in mapped:
                    fl.lift_mapped(e)                    # (returns once the pose is in host memory)
            dt = (time.perf_counter() - t0) / reps_loop
            out["loop_us"].append(round(1e6 * dt, 1))
            out["loop_fps"].append(round(n / dt))
        out["speedup"] = round(float(np.median(out["clip_fps"]) / np.median(out["loop_fps"])), 2)
        print(json.dumps(out), flush=True)
    m.check_errors()
    m.close()
    for n in (4096, 1 << 16, 1 << 20):
        print(json.dumps(device_times(n, 50, rng)), flush=True)


if __name__ == "__main__":
    main()
