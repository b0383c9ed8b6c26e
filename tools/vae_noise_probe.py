"""Dev tool: device times of the noise kernel (csrc/p3d_vae_noise.h k_vae_noise) and what it replaces
in the drivers, one JSON line per measurement, also appended to profiles/vae_noise_probe.jsonl.

  (a) k_vae_noise at 2^20 rows, widths 48 and 144, in the plain form (out of place and in place) and
      the window form (48-float frames, the starts a permutation), at the default threshold and --
      through p3d_vae_add_noise_thr -- with every row noised and with none: time, bytes moved
      (read + written, 8 bytes per element; in place only the noised rows move) over time against
      8 TB/s, and normals per second (noised rows x (width + 4)) against k_vae_eps at [2^20, 48] in
      the same run, alternated round by round;
  (b) one epoch's noise preparation of 3d_pose_vae_filter_kin.train at 2^20 windows: the host path
      (gather, .cpu(), add_noise, .to(device)) on the host clock around a synchronize against one
      add_noise_device call, beside that epoch's 16,384 training steps at batch 64;
  (c) the epoch loop body of vae_filter.train (two Dataset gathers and one training step per batch)
      over one synthetic epoch of 2^18 poses: steps per second.

    python tools/vae_noise_probe.py [--rounds 5] [--reps 20]
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
from top_vae_3d_pose import data_handler, models  # noqa: E402

HBM_PEAK = 8.0e12        # bytes / s (MI355X)
P_NOISED = 0.30853753872598694
ENC, LAT, DEC = (40, 32), 24, (32, 40)
FACTORS = (100.0, 0.02, 1.0)
SEED = 7


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps      # microseconds per call


def noise_call(src, starts, width, out, thr):
    rows, d = src.shape
    B = out.shape[0]
    scale = float(data_handler.joint_scale([1, 1]))
    lib, st = _p3d.lib(), _p3d.ptr(starts) or None

    def fn():
        _p3d.check(lib.p3d_vae_add_noise_thr(_p3d.ptr(src), rows, d, st, width, B, SEED, 1, 0, data_handler.NOISE,
                                             data_handler.NOISE_OFFSET, scale, thr, _p3d.ptr(out), _p3d.stream_handle()),
                   "p3d_vae_add_noise_thr")
    return fn


def main():
    arg = lambda k, d: int(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d   # noqa: E731
    rounds, reps = arg("--rounds", 5), arg("--reps", 20)
    assert torch.cuda.is_available(), "the probe needs a GPU"
    dev = torch.device("cuda")
    out = []
    n = 1 << 20

    # (a) the kernel
    eps_out = torch.empty((n, 48), dtype=torch.float32, device=dev)
    eps = lambda: _p3d.check(_p3d.lib().p3d_vae_eps(SEED, 1, 0, n, 48, _p3d.ptr(eps_out), _p3d.stream_handle()),   # noqa: E731
                             "p3d_vae_eps")
    frames = torch.randn((n + 2, 48), device=dev)
    perm = torch.randperm(n, device=dev)
    cases = {"k_vae_eps_2^20x48": (eps, n * 48, n * 48 * 4)}
    keep = []
    for width in (48, 144):
        x = torch.randn((n, width), device=dev)
        o = torch.empty_like(x)
        xi = x.clone()
        keep += [x, o, xi]
        for tag, thr, share in (("default", 0xB103AF11, P_NOISED), ("all", 0, 1.0), ("none", 1 << 32, 0.0)):
            normals = int(round(n * share)) * (width + 4)
            cases["plain_w%d_%s" % (width, tag)] = (noise_call(x, None, width, o, thr), normals, 2 * n * width * 4)
            cases["window_w%d_%s" % (width, tag)] = (noise_call(frames, perm, width, o, thr), normals, 2 * n * width * 4 + 8 * n)
        cases["inplace_w%d_default" % width] = (noise_call(xi, None, width, xi, 0xB103AF11),
                                                int(round(n * P_NOISED)) * (width + 4),
                                                int(round(n * P_NOISED)) * 2 * width * 4)
    for fn, _, _ in cases.values():
        timed(fn, 3)
    us = {k: [] for k in cases}
    for _ in range(rounds):
        for k, (fn, _, _) in cases.items():
            us[k].append(round(timed(fn, reps), 2))
    eps_rate = None
    for k, (fn, normals, nbytes) in cases.items():
        med = float(np.median(us[k]))
        rec = {"what": k, "rows": n, "us": us[k], "us_median": med, "bytes": nbytes,
               "GBps": round(nbytes / med / 1e3, 1), "share_of_hbm_peak": round(1e6 * nbytes / HBM_PEAK / med, 3),
               "normals": normals, "Gnormals_per_s": round(normals / med / 1e3, 2), "reps": reps, "rounds": rounds}
        if k.startswith("k_vae_eps"):
            eps_rate = rec["Gnormals_per_s"]
        elif normals:
            rec["normals_rate_vs_k_vae_eps"] = round(rec["Gnormals_per_s"] / eps_rate, 3)
        out.append(rec)
    del keep, cases, eps_out
    torch.cuda.empty_cache()

    # (b) one epoch's noise preparation of the temporal driver at 2^20 windows
    size, seq = 48, 3
    starts = perm.clone()
    cols = torch.arange(seq * size, device=dev)

    def host_path():
        X = frames.view(-1)[(starts * size)[:, None] + cols[None, :]]
        return torch.from_numpy(data_handler.add_noise(X.cpu().numpy(), [1, 1])).to(dev)

    def device_path():
        return data_handler.add_noise_device(frames, [1, 1], starts=starts, width=seq * size, seed=SEED, ctr=1)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    wall(device_path)
    np.random.seed(0)
    host_s = [round(wall(host_path), 4) for _ in range(3)]
    dev_s = [round(wall(device_path), 6) for _ in range(5)]
    dev_us = [round(timed(device_path, 5), 1) for _ in range(3)]      # (allocates its [2^20, 144] result inside)
    m = models.VAE(seq * size, LAT, ENC, DEC, human_3d_size=size, max_batch=4096, seed=3)
    X = device_path()
    Y = frames[starts + (seq - 1)]
    loss = torch.zeros((n // 64, 3), device=dev)

    def epoch_steps():
        for s in range(n // 64):
            m.train_step_device(X[s * 64:(s + 1) * 64], Y[s * 64:(s + 1) * 64], FACTORS, 1e-4, loss_out=loss[s])

    wall(lambda: [m.train_step_device(X[:64], Y[:64], FACTORS, 1e-4, loss_out=loss[0]) for _ in range(200)])
    steps_s = [round(wall(epoch_steps), 4) for _ in range(2)]
    out.append({"what": "kin_epoch_noise_preparation_2^20_windows", "host_path_s": host_s,
                "host_path_s_median": float(np.median(host_s)), "add_noise_device_wall_s": dev_s,
                "add_noise_device_wall_s_median": float(np.median(dev_s)), "add_noise_device_event_us": dev_us,
                "ratio_host_over_device": round(float(np.median(host_s)) / float(np.median(dev_s)), 1),
                "epoch_16384_steps_s": steps_s, "bytes_each_way_host_path": n * seq * size * 4})
    m.close()
    del X, Y

    # (c) vae_filter.train's loop body over one synthetic epoch
    n2 = 1 << 18
    ds = data_handler.Dataset(torch.randn((n2, 48), device=dev), batch_size=64, seed=SEED)
    m = models.VAE(48, LAT, ENC, DEC, max_batch=4096, seed=3)
    loss = torch.zeros((len(ds), 3), device=dev)

    def epoch():
        for step, (xn, xt) in enumerate(ds):
            m.train_step_device(xn, xt, FACTORS, 1e-4, loss_out=loss[step])
        ds.on_epoch_end(new_noise=True)

    wall(epoch)
    ep = [round(wall(epoch), 4) for _ in range(3)]
    out.append({"what": "vae_filter_epoch_loop_2^18_poses", "steps": len(ds), "epoch_s": ep,
                "steps_per_s": round(len(ds) / float(np.median(ep)), 1),
                "us_per_step": round(1e6 * float(np.median(ep)) / len(ds), 2),
                "note": "two device gathers + one p3d_vae_train_step per batch of 64, the epoch's re-noise included"})
    m.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "vae_noise_probe.jsonl"), "a") as f:
        for rec in out:
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
