"""Dev tool: device times of the VAE filter averaged over K posterior samples (csrc/p3d_vae_mc.h),
one JSON line per measurement, also appended to profiles/vae_mc_probe.jsonl.

In one process, device events around `reps` back-to-back calls, the cases of one measurement
alternated over `rounds` rounds after a warm-up, every round's figure and the median reported:

  (a) p3d_vae_forward_mc on the default filter (48 -> 40 -> 32 -> {24, 24} -> 32 -> 40 -> 48) at 2^20
      rows and at 64 rows for K in {1, 4, 16}, the caller's eps, y_mean and y_var written, against
      the composition it replaces over the same rows: K p3d_vae_forward launches into one y buffer
      and the fold of include/p3d.h written with torch elementwise operations into preallocated
      buffers.  The two are asserted bit-equal before anything is timed.  At K = 1 the plain
      p3d_vae_forward launch is timed beside them: what the fold's scaffolding costs.
  (b) p3d_vae_seq_filter_mc (k_vae_seq4_mc) over the H3.6M test split's shape of
      tools/vae_seq_probe.py (S = 240 sequences, lengths uniform in [1500, 3000], seed 2024, the
      144-input filter, the caller's eps) for K in {1, 4, 16}, beside k_vae_seq4 (form 1 of
      p3d_vae_seq_filter) in the same run.  A launch runs as many frame steps as its longest
      sequence has frames; the time per frame step is the launch time over that count.  K = 1 is
      asserted bit-equal to k_vae_seq4 first.

    python tools/vae_mc_probe.py [--rounds 5] [--reps 3]
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

KS = (1, 4, 16)
S, LO, HI = 240, 1500, 3000


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps      # microseconds per call


def run_cases(cases, rounds, reps):
    for fn in cases.values():                    # warm-up
        fn()
        fn()
    torch.cuda.synchronize()
    us = {k: [] for k in cases}
    for _ in range(rounds):                      # alternate the cases round by round
        for k, fn in cases.items():
            us[k].append(round(timed(fn, reps), 2))
    return us


def emit(rec, us):
    for k, v in us.items():
        rec[k + "_us"] = v
        rec[k + "_us_median"] = float(np.median(v))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(os.path.join(ROOT, "profiles", "vae_mc_probe.jsonl"), "a") as f:
        f.write(line + "\n")
    return rec


def c(k):
    return float(np.float32(1.0 / (k + 1)))


def forward_cases(vae, B, rounds, reps):
    lib, st, ptr = _p3d.lib(), _p3d.stream_handle, _p3d.ptr
    x = torch.randn((B, 48), device="cuda")
    eps = torch.randn((max(KS), B, 24), device="cuda")
    ym, yv = torch.empty((B, 48), device="cuda"), torch.empty((B, 48), device="cuda")
    y, m, M, d, t = (torch.empty((B, 48), device="cuda") for _ in range(5))
    var = torch.empty((B, 48), device="cuda")

    def plain(k, out):
        _p3d.check(lib.p3d_vae_forward(vae._h, ptr(x), B, ptr(eps[k]), 0, ptr(out), None, None, None, None, None, st()),
                   "p3d_vae_forward")

    for K in KS:
        def mc():
            _p3d.check(lib.p3d_vae_forward_mc(vae._h, ptr(x), B, K, ptr(eps), 0, ptr(ym), ptr(yv), None, None, st()),
                       "p3d_vae_forward_mc")

        def composition():
            plain(0, m)
            M.zero_()
            for k in range(1, K):
                plain(k, y)
                torch.sub(y, m, out=d)
                torch.mul(d, c(k), out=t)
                m.add_(t)
                torch.sub(y, m, out=t)
                t.mul_(d)
                M.add_(t)
            torch.mul(M, c(K - 1), out=var)

        mc()
        composition()
        torch.cuda.synchronize()
        assert torch.equal(ym, m) and torch.equal(yv, var), "forward_mc differs from the composition at K = %d" % K
        cases = {"forward_mc": mc, "composition": composition}
        if K == 1:
            cases["forward_plain"] = lambda: plain(0, y)
        us = run_cases(cases, rounds, reps)
        rec = {"what": "vae_forward_mc", "B": B, "K": K, "rounds": rounds, "reps": reps}
        rec = emit(rec, us)
        print("  forward B %d K %d: mc %.1f us, composition %.1f us (%.2fx)" % (
            B, K, rec["forward_mc_us_median"], rec["composition_us_median"],
            rec["composition_us_median"] / rec["forward_mc_us_median"]), flush=True)


def sequence_cases(rounds, reps):
    lib, st, ptr = _p3d.lib(), _p3d.stream_handle, _p3d.ptr
    rng = np.random.default_rng(2024)
    lens = rng.integers(LO, HI + 1, size=S)
    off_h = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N, tmax = int(off_h[-1]), int(lens.max())
    vae = models.VAE(144, 24, [40, 32], [32, 40], max_batch=1024, seed=3)
    pred = torch.randn((N, 48), device="cuda")
    eps = torch.randn((max(KS), N, 24), device="cuda")
    off = torch.from_numpy(off_h).cuda()
    ref, var, ref0 = (torch.empty((N, 48), device="cuda") for _ in range(3))

    def seq4():
        _p3d.check(lib.p3d_vae_seq_filter(vae._h, ptr(pred), ptr(off), S, N, ptr(eps[0]), 0, 0, None, None, None,
                                          ptr(ref0), None, None, st()), "p3d_vae_seq_filter")

    def mc(K):
        def run():
            _p3d.check(lib.p3d_vae_seq_filter_mc(vae._h, ptr(pred), ptr(off), S, N, K, ptr(eps), 0, 0, None, None, None,
                                                 ptr(ref), ptr(var), None, None, st()), "p3d_vae_seq_filter_mc")
        return run

    seq4()
    mc(1)()
    torch.cuda.synchronize()
    assert torch.equal(ref, ref0) and not var.any(), "k_vae_seq4_mc at K = 1 differs from k_vae_seq4"
    cases = {"seq4": seq4}
    cases.update({"seq4_mc_K%d" % K: mc(K) for K in KS})
    us = run_cases(cases, rounds, reps)
    rec = {"what": "vae_seq4_mc_h36m_shape", "S": S, "N": N, "longest": tmax, "tiles": (S + 15) // 16,
           "rounds": rounds, "reps": reps}
    for k, v in us.items():
        rec[k + "_us_per_frame_step"] = round(float(np.median(v)) / tmax, 3)
    emit(rec, us)
    vae.close()


def main():
    arg = lambda k, d: int(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d   # noqa: E731
    rounds, reps = arg("--rounds", 5), arg("--reps", 3)
    vae = models.VAE(48, 24, [40, 32], [32, 40], max_batch=4096, seed=3)
    forward_cases(vae, 1 << 20, rounds, reps)
    forward_cases(vae, 64, rounds, max(reps, 50))       # (a 64-row call is a few microseconds: more of them a window)
    vae.close()
    sequence_cases(rounds, reps)


if __name__ == "__main__":
    main()
