"""Time the spline resampling (MEASUREMENTS.md 30) on the GPU: p3d_clips_resample alone,
and p3d_clips_lift_resampled beside p3d_clips_lift on the same clips, at R = 10 for one clip of 300
frames and for 240 clips of 300 frames.  One JSON line per measurement on stdout.

    python tools/spline_probe.py [--iters 3] [--scipy]

--scipy (where scipy is installed; no GPU needed for it) times the reference's own two calls per curve
on the same tracks, on the CPU, for the figure that stands beside the kernel's.

The tracks are smooth motion with detector noise (amplitude 50 px, noise 1 px), smoothed by the clip
kernels first; the model is a fresh 1024 x 2 lifter.  Times are medians of --iters runs after one
warm-up, taken with events on the stream (the calls are asynchronous)."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-pose-baseline_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def clips_for(S, m=300, seed=0):
    rng = np.random.default_rng(seed)
    x = np.arange(m)[:, None]
    out = []
    for _ in range(S):
        ph = rng.uniform(0, 6.28, (2, 36))
        amp = rng.uniform(5.0, 50.0, 36)
        out.append(600.0 + amp * np.sin(x * 0.07 + ph[0]) + 0.3 * amp * np.sin(x * 0.31 + ph[1])
                   + rng.standard_normal((m, 36)))
    return out


def scipy_times(clips):
    from scipy.interpolate import UnivariateSpline
    t0 = time.perf_counter()
    n = 0
    for xy in clips:
        m = xy.shape[0]
        at = np.arange(0, m, 0.1)
        for col in range(36):
            y = [float(v) for v in xy[:, col]]
            spl = UnivariateSpline(range(m), y, k=3)
            spl.set_smoothing_factor(float((max(y) - min(y)) * 125))
            spl(at)
            n += 1
    dt = time.perf_counter() - t0
    return dict(what="scipy UnivariateSpline + set_smoothing_factor + call, CPU", curves=n, seconds=dt, ms_per_curve=1e3 * dt / n)


def timed(torch, fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--scipy", action="store_true")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 240])
    f = ap.parse_args(argv)
    if f.scipy:
        print(json.dumps(scipy_times(clips_for(1))), flush=True)
        return
    import torch
    import _p3d
    import data_utils
    import linear_model
    import openpose_frontend as of
    from oracle import ref_mlp
    R = 10
    use2, _ = data_utils.dimension_sets(2)
    _, ign3 = data_utils.dimension_sets(3)
    rng = np.random.default_rng(3)
    st = ref_mlp.init_state(ref_mlp.Cfg(linear_size=1024, num_layers=2, residual=True, batch_norm=True), seed=3, bn_seed=4)
    model = linear_model.LinearModel(1024, 2, True, True, False, 64, 1e-3, "/tmp/p3d_spline_probe", seed=11)
    model.set_weights({**st.params, **st.moving})
    stats = (rng.uniform(200, 600, 64), rng.uniform(50, 150, 64), use2, rng.uniform(-400, 400, 96), rng.uniform(30, 300, 96), ign3)
    for S in f.batches:
        clips = clips_for(S)
        N = 300 * S
        cl = of.ClipLifter(model, *stats, max_frames=N)
        cl.hin.numpy()[:N] = np.concatenate(clips)
        cl.set_offsets(np.arange(S + 1, dtype=np.int64) * 300)
        cl.din[:N].copy_(cl.hin[:N])
        t_lift = timed(torch, lambda: cl.lift_clips_device(True), f.iters)
        t_res = timed(torch, lambda: cl.lift_clips_resampled_device(R, True), f.iters)
        rs, p, lib = cl.resampled.d, _p3d.ptr, _p3d.lib()
        nb = int(lib.p3d_clips_resample_workspace(N, S, R))
        work = torch.empty((nb // 8 + 32,), dtype=torch.float64, device="cuda")
        wp = (work.data_ptr() + 255) // 256 * 256
        x = torch.empty((R * N, len(use2)), dtype=torch.float32, device="cuda")

        def alone():
            _p3d.check(lib.p3d_clips_resample(p(cl.dxy), cl._off.ctypes.data, p(cl.doff), S, N, R, p(cl.m2), p(cl.s2), p(cl.u2),
                                              cl.u2.numel(), p(x), p(rs["xy"]), p(rs["off"]), p(rs["info"]), wp, nb,
                                              model.stream()), "p3d_clips_resample")
        t_alone = timed(torch, alone, f.iters)
        info = rs["info"][:S].cpu().numpy().reshape(-1, 5)
        print(json.dumps(dict(clips=S, frames=300, R=R, curves=36 * S, p3d_clips_lift_ms=t_lift,
                              p3d_clips_lift_resampled_ms=t_res, p3d_clips_resample_ms=t_alone,
                              resample_ms_per_curve=t_alone / (36 * S), workspace_MiB=nb / 2 ** 20,
                              knots_mean=float(info[:, 1].mean()), knots_max=int(info[:, 1].max()),
                              p_iterations_mean=float(info[:, 4].mean()),
                              ier2_counts={str(k): int((info[:, 3] == k).sum()) for k in np.unique(info[:, 3])})), flush=True)
        del cl, work, x
    model.close()


if __name__ == "__main__":
    main()
