"""Dev tool: what a tick of the live path costs (openpose_frontend.LiveLifter, p3d_live_push), per
tick from the call to the result on the host, at steady state, all in one process:

  * S = 1, no smoothing, no filter, against FrameLifter.lift on a raw frame (the batch-1 path the
    live front end had before) and against p3d_empty_launch (device events around back-to-back
    launches: the launch floor).  A plain tick has two launches more than FrameLifter's one (k_live_in,
    k_live_out) and a signal launch for the completion word: `excess_us` is how far it sits above
    FrameLifter.lift plus two empty launches.
  * S = 1 and S = 64 with smoothing and the temporal filter (one draw, and K = 4), against what the
    clip path offers for the same poses: ClipLifter.lift_clips over the streams' frames so far,
    taken at 256 frames in.

Host wall-clock (time.perf_counter) around every call, medians over the timed calls.  One JSON line
per measurement, appended to profiles/live_probe.jsonl (--out PATH: another file).

    python tools/live_probe.py [--ticks 200] [--out PATH]
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
import data_utils  # noqa: E402
import linear_model  # noqa: E402
import openpose_frontend as of  # noqa: E402
from top_vae_3d_pose import models  # noqa: E402


def wall_us(fn, n, warm):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(t)), float(np.percentile(t, 90))


def frames(rng, n):
    xy = rng.uniform(100, 900, (n, 36))
    xy[rng.random((n, 36)) < 0.2] = 0.0                  # dropped joints, as OpenPose leaves them
    xy[:, 2:4] = rng.uniform(540, 700, (n, 2))
    return xy


def main():
    arg = lambda k, d, t=int: t(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d   # noqa: E731
    n_ticks = arg("--ticks", 200)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "live_probe.jsonl"), str)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    rng = np.random.default_rng(901)
    m = linear_model.LinearModel(1024, 2, True, True, False, 64, 1e-3, "/tmp/p3d_live_probe", seed=5, max_batch=8192)
    vae = models.VAE(144, 24, [40, 32], [32, 40], max_batch=1024, seed=3)
    use2, _ = data_utils.dimension_sets(2)
    _, ign3 = data_utils.dimension_sets(3)
    stats = (rng.uniform(200, 600, 64), rng.uniform(50, 150, 64), use2, rng.uniform(-400, 400, 96),
             rng.uniform(30, 300, 96), ign3)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")

    # ---- the plain tick against FrameLifter.lift and the launch floor
    xy = frames(rng, 64)
    fl = of.FrameLifter(m, *stats, batch=1)
    live = of.LiveLifter(m, *stats, slots=1, smooth=False)
    slot, k = live.open(), [0]

    def tick():
        live.push({slot: xy[k[0] & 63]})
        k[0] += 1

    def frame():
        fl.lift(xy[k[0] & 63])
        k[0] += 1

    lib, sh = _p3d.lib(), _p3d.stream_handle
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    empty = []
    for _ in range(5):
        e0.record()
        for _ in range(200):
            lib.p3d_empty_launch(m._h, 1, sh())
        e1.record()
        torch.cuda.synchronize()
        empty.append(e0.elapsed_time(e1) * 1000 / 200)
    empty_us = float(np.median(empty))
    rec = {"what": "live_plain_tick_vs_frame_lifter", "S": 1, "smooth": 0, "ticks": n_ticks, "live_us": [], "frame_us": []}
    for _ in range(3):                                    # alternate: live, frame, live, frame, ...
        rec["live_us"].append(round(wall_us(tick, n_ticks, 50)[0], 2))
        rec["frame_us"].append(round(wall_us(frame, n_ticks, 50)[0], 2))
    rec["empty_launch_us"] = round(empty_us, 2)
    rec["excess_us"] = round(float(np.median(rec["live_us"]) - np.median(rec["frame_us"]) - 2 * empty_us), 2)
    emit(rec)
    live.close(slot)

    # ---- smoothing and the filter, S streams, against lift_clips over the frames so far at 256 in
    for S in (1, 64):
        streams = [frames(rng, 256) for _ in range(S)]
        cl = of.ClipLifter(m, *stats, max_frames=256 * S)
        for K in (None, 4):
            live = of.LiveLifter(m, *stats, slots=S, vae=vae, samples=K)
            slots = [live.open() for _ in range(S)]
            t = []
            for f in range(256):
                rows = {s: streams[i][f] for i, s in enumerate(slots)}
                t0 = time.perf_counter()
                live.push(rows)
                t.append((time.perf_counter() - t0) * 1e6)
            steady = t[256 - min(n_ticks, 200):]
            clip = wall_us(lambda: cl.lift_clips(streams, vae=vae, samples=K), 5, 2)
            emit({"what": "live_tick_vs_lift_clips_so_far", "S": S, "smooth": 1, "K": K, "frames_in": 256,
                  "live_tick_us": round(float(np.median(steady)), 2), "live_tick_p90_us": round(float(np.percentile(steady, 90)), 2),
                  "lift_clips_us": round(clip[0], 2),
                  "speedup": round(clip[0] / float(np.median(steady)), 1)})
            live.push({}, close=slots)
        del cl
    m.check_errors()
    vae.close()
    m.close()


if __name__ == "__main__":
    main()
