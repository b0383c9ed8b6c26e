"""Dev tool: device times of the temporal filter's recurrence over whole sequences
(csrc/p3d_vae_seq.h), one JSON line per measurement, also appended to profiles/vae_seq_probe.jsonl.

The input has the shape of the H3.6M test split: S = 240 sequences with lengths uniform in
[1500, 3000] (seed fixed), the 144 -> 40 -> 32 -> {24, 24} -> 32 -> 40 -> 48 filter, the caller's eps.

  * k_vae_seq in form 0 (one wave per 16-sequence tile) and form 1 (four waves per tile) over the
    whole set: device events around `reps` back-to-back calls, the two alternated over `rounds`
    rounds after a warm-up, medians reported.  A launch runs as many frame steps as its longest
    sequence has frames; the time per frame step is the launch time over that count.
  * the per-frame path: one p3d_vae_forward of S rows per frame with the window assembled by one
    torch.cat between calls, over the first 256 frames of every sequence (every sequence is longer
    than that, so each step serves all S rows), reported per frame.
  * before timing, form 0 == form 1 and both == the per-frame path on those 256 frames, bit for bit.

    python tools/vae_seq_probe.py [--rounds 5] [--reps 3]
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
from top_vae_3d_pose import models  # noqa: E402

S, LO, HI, BASE_FRAMES = 240, 1500, 3000, 256


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
    rounds, reps = arg("--rounds", 5), arg("--reps", 3)
    rng = np.random.default_rng(2024)
    lens = rng.integers(LO, HI + 1, size=S)
    off_h = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N, tmax = int(off_h[-1]), int(lens.max())
    vae = models.VAE(144, 24, [40, 32], [32, 40], max_batch=1024, seed=3)
    pred = torch.randn((N, 48), device="cuda")
    eps = torch.randn((N, 24), device="cuda")
    off = torch.from_numpy(off_h).cuda()
    ref = torch.empty((N, 48), device="cuda")
    lib, st = _p3d.lib(), _p3d.stream_handle
    ptr = _p3d.ptr

    def seq():
        _p3d.check(lib.p3d_vae_seq_filter(vae._h, ptr(pred), ptr(off), S, N, ptr(eps), 0, 0, None, None, None, ptr(ref),
                                          None, None, st()), "p3d_vae_seq_filter")

    def form(k):
        def run():
            vae.set_seq_form(k)
            seq()
        return run

    # the per-frame path: frame-major copies of the first frames, two window buffers used in turn
    idx = (off[:-1, None] + torch.arange(BASE_FRAMES, device="cuda")[None, :]).t().contiguous()    # [F, S]
    pf, ef = pred[idx], eps[idx]                          # [F, S, 48], [F, S, 24]
    yf = torch.empty((BASE_FRAMES, S, 48), device="cuda")
    xs = [torch.empty((S, 144), device="cuda") for _ in range(2)]

    def per_frame():
        torch.cat((pf[0], pf[0], pf[0]), dim=1, out=xs[0])
        for f in range(BASE_FRAMES):
            x = xs[f & 1]
            _p3d.check(lib.p3d_vae_forward(vae._h, ptr(x), S, ptr(ef[f]), 0, ptr(yf[f]), None, None, None, None, None,
                                           st()), "p3d_vae_forward")
            if f + 1 < BASE_FRAMES:
                torch.cat((x[:, 48:96], yf[f], pf[f + 1]), dim=1, out=xs[(f + 1) & 1])

    # ---- the three paths agree before anything is timed ----
    form(0)()
    r0 = ref.clone()
    form(1)()
    per_frame()
    torch.cuda.synchronize()
    assert torch.equal(ref, r0), "form 1 differs from form 0"
    assert torch.equal(yf, r0[idx]), "the per-frame path differs from the one-launch path"
    cases = {"form0": form(0), "form1": form(1), "per_frame_loop": per_frame}
    for fn in cases.values():                            # warm-up
        fn()
        fn()
    torch.cuda.synchronize()
    us = {k: [] for k in cases}
    for _ in range(rounds):                              # alternate the cases round by round
        for k, fn in cases.items():
            us[k].append(round(timed(fn, reps), 1))
    med = {k: float(np.median(v)) for k, v in us.items()}
    rec = {"what": "vae_seq_h36m_shape", "S": S, "N": N, "longest": tmax, "tiles": (S + 15) // 16, "rounds": rounds,
           "reps": reps, "base_frames": BASE_FRAMES}
    for k, v in us.items():
        rec[k + "_us"] = v
        rec[k + "_us_median"] = med[k]
    rec["form0_us_per_frame_step"] = round(med["form0"] / tmax, 3)
    rec["form1_us_per_frame_step"] = round(med["form1"] / tmax, 3)
    rec["per_frame_loop_us_per_frame"] = round(med["per_frame_loop"] / BASE_FRAMES, 3)
    rec["form0_ns_per_sequence_frame"] = round(1e3 * med["form0"] / N, 3)
    rec["form1_ns_per_sequence_frame"] = round(1e3 * med["form1"] / N, 3)
    rec["faster_form"] = 0 if med["form0"] <= med["form1"] else 1
    best = min(rec["form0_us_per_frame_step"], rec["form1_us_per_frame_step"])
    rec["one_launch_over_per_frame_loop"] = round(rec["per_frame_loop_us_per_frame"] / best, 2)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(os.path.join(ROOT, "profiles", "vae_seq_probe.jsonl"), "a") as f:
        f.write(line + "\n")
    vae.close()


if __name__ == "__main__":
    main()
