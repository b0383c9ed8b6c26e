"""Dev tool: a batch of OpenPose clips through ONE p3d_clips_lift (ClipLifter.lift_clips_device)
against a loop of the existing per-clip calls over the same device rows -- p3d_clip_lift per clip
and, with the temporal filter, p3d_vae_seq_filter(_mc) at S = 1 and p3d_clip_finish behind it --
in one process, the two alternated over `rounds` after a warm-up, device events around `reps`
back-to-back passes (the loop's host time between its launches is part of what it costs and is
inside its events).  Without a filter, with the filter at one draw, and at K = 4.  Before timing,
the probe asserts that both sides leave the same bits.  One JSON line per measurement, appended
to profiles/clips_probe.jsonl (--out PATH: another file).

Workloads: the 240 sequence lengths of the H3.6M test split's shape (uniform in [1500, 3000], seed
2024: 524,599 frames), 64 clips x 256 frames, and 1,000 clips x 9 frames (the forward is tiled
clip by clip, so this one is bound by its launches).

    python tools/clips_probe.py [--rounds 3] [--only h36m|64x256|1000x9] [--out PATH]
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
import data_utils  # noqa: E402
import linear_model  # noqa: E402
import openpose_frontend as of  # noqa: E402
from top_vae_3d_pose import models  # noqa: E402


def workloads():
    rng = np.random.default_rng(2024)
    return {"h36m": rng.integers(1500, 3001, size=240), "64x256": np.full(64, 256), "1000x9": np.full(1000, 9)}


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def per_clip_loop(cl, vae, K, off, ctr):
    """The existing calls clip by clip on slices of the lifter's device buffers; returns the pass."""
    lib, m = _p3d.lib(), cl.model
    S = len(off) - 1
    pairs = torch.tensor([[0, int(off[s + 1] - off[s])] for s in range(S)], dtype=torch.int64, device=m.device)
    ref = torch.empty((int(off[-1]), 48), dtype=torch.float32, device=m.device)
    var = torch.empty_like(ref) if K else None
    st = (cl.m2.data_ptr(), cl.s2.data_ptr(), cl.u2.data_ptr(), cl.u2.numel(), cl.m3.data_ptr(), cl.s3.data_ptr(),
          cl.u3.data_ptr(), cl.u3.numel(), 96, int(cl.cache_on_fail))
    calls = []
    for s in range(S):
        a, n = int(off[s]), int(off[s + 1] - off[s])
        outs = (cl.dxy.data_ptr() + a * 288, cl.dout.data_ptr() + a * 768, cl.dsrc.data_ptr() + a * 4)
        lift = (m._h, cl.din.data_ptr() + a * 288, n, 1) + st + outs + (cl.work_ptr, cl.work_bytes)
        wb = int(lib.p3d_clip_workspace(n))
        y = cl.work_ptr + of.lift_layout(wb, n, m.input_size, m.output_size)[1]
        r = ref.data_ptr() + a * 192
        flt = (vae._h, y, pairs.data_ptr() + 16 * s, 1, n) if vae is not None else None
        fin = (r, n, outs[0]) + st[4:] + outs[1:] + (cl.work_ptr, wb)
        calls.append((lift, flt, fin, a, r, None if var is None else var.data_ptr() + a * 192))

    def run():
        h = m.stream()
        for lift, flt, fin, a, r, v in calls:
            rc = lib.p3d_clip_lift(*lift, h)
            if flt is not None:
                if K:
                    rc |= lib.p3d_vae_seq_filter_mc(*flt, K, None, ctr, a, None, None, None, r, v, None, None, h)
                else:
                    rc |= lib.p3d_vae_seq_filter(*flt, None, ctr, a, None, None, None, r, None, None, h)
                rc |= lib.p3d_clip_finish(*fin, h)
            if rc:
                _p3d.check(rc, "the per-clip loop")
    return run, (ref, var, pairs)


def main():
    arg = lambda k, d, t=int: t(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d   # noqa: E731
    rounds, only = arg("--rounds", 3), arg("--only", None, str)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "clips_probe.jsonl"), str)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    rng = np.random.default_rng(900)
    m = linear_model.LinearModel(1024, 2, True, True, False, 64, 1e-3, "/tmp/p3d_clips_probe", seed=5, max_batch=8192)
    vae = models.VAE(144, 24, [40, 32], [32, 40], max_batch=1024, seed=3)
    use2, _ = data_utils.dimension_sets(2)
    _, ign3 = data_utils.dimension_sets(3)
    stats = (rng.uniform(200, 600, 64), rng.uniform(50, 150, 64), use2, rng.uniform(-400, 400, 96),
             rng.uniform(30, 300, 96), ign3)
    for name, lens in workloads().items():
        if only and name != only:
            continue
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        S, N = len(lens), int(off[-1])
        cl = of.ClipLifter(m, *stats, max_frames=N)
        xy = rng.uniform(100, 900, (N, 36))
        xy[rng.random((N, 36)) < 0.2] = 0.0              # dropped joints, as OpenPose leaves them
        cl.din.copy_(torch.from_numpy(xy))
        cl.set_offsets(off)
        row_off = torch.repeat_interleave(torch.from_numpy(off[:-1]), torch.from_numpy(np.asarray(lens))).to(m.device).int()
        for label, v, K in (("no_filter", None, None), ("filter", vae, None), ("filter_K4", vae, 4)):
            batched = lambda: cl.lift_clips_device(True, v, K, None, 5, 0, False)   # noqa: E731
            loop, keep = per_clip_loop(cl, v, K, off, 5)
            loop()                                        # warm-up, and the check: the same bits
            torch.cuda.synchronize()
            src = cl.dsrc[:N].clone()                     # (the loop's are positions inside the clip)
            want = (cl.dout[:N].clone(), cl.dxy[:N].clone(), torch.where(src >= 0, src + row_off, src))
            for t in (cl.dout, cl.dxy):
                t.fill_(3.0)
            batched()
            torch.cuda.synchronize()
            for got, w in zip((cl.dout, cl.dxy, cl.dsrc), want):
                assert got[:N].view(torch.uint8).equal(w.view(torch.uint8)), "%s %s: the batch and the loop differ" % (name, label)
            m.check_errors()
            # the per-clip loop with the filter runs S serial chains: one pass is enough to time it
            reps_b = 3
            reps_l = 1 if (v is not None and N > 100000) else 3
            rec = {"what": "clips_batched_vs_per_clip_loop", "workload": name, "S": S, "N": N, "case": label,
                   "reps": [reps_b, reps_l], "batched_ms": [], "loop_ms": []}
            for _ in range(rounds):                       # alternate: batch, loop, batch, loop, ...
                rec["batched_ms"].append(round(timed(batched, reps_b), 3))
                rec["loop_ms"].append(round(timed(loop, reps_l), 3))
            rec["speedup"] = round(float(np.median(rec["loop_ms"]) / np.median(rec["batched_ms"])), 2)
            line = json.dumps(rec)
            print(line, flush=True)
            with open(out_path, "a") as f:
                f.write(line + "\n")
            del keep
        del cl
        torch.cuda.empty_cache()
    m.check_errors()
    vae.close()
    m.close()


if __name__ == "__main__":
    main()
