"""Dev tool: p3d_root_trajectory at 2^20 rows, as one clip and as 240 clips, at smooth_half 0 and 4
(all four outputs; the solve alone with traj_raw only), device events around `reps` back-to-back
calls after a warm-up, against the bytes each must move: N (768 + 288 + the outputs asked for).  In
the same run at the same N: p3d_clip_finish (k_clip_out: the same rows written that this call
reads), p3d_skel_pose with the root only (the same poses rows in, 24 bytes out), and the numpy
oracle (tests/traj_oracle.py) on the host -- its solve over all rows, its Python window loop over
the first 2^14.  One JSON line per measurement, appended to profiles/traj_probe.jsonl (--out PATH:
another file).

    python tools/traj_probe.py [--reps 20] [--n 1048576] [--out PATH] [--no-oracle]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-pose-baseline_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _p3d  # noqa: E402
import traj_oracle as to  # noqa: E402
from tools.skel_probe import BYTES as SKEL_BYTES, clip_finish_call, timed_us  # noqa: E402

ROW_IN = 96 * 8 + 36 * 8                       # the poses row and the xy_s row of a frame
OUT_BYTES = {"traj": 24, "traj_raw": 24, "resid": 8, "valid": 4}


def main():
    arg = lambda k, d, t=int: t(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d   # noqa: E731
    reps, N = arg("--reps", 20), arg("--n", 1 << 20)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "traj_probe.jsonl"), str)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    lib, p, st = _p3d.lib(), _p3d.ptr, _p3d.stream_handle
    rng = np.random.default_rng(901)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")

    def rate(what, S, h, us, per_row, **more):
        emit(dict({"what": what, "N": N, "S": S, "h": h, "reps": reps, "us": round(us, 2), "bytes": N * per_row,
                   "GBps": round(N * per_row / us / 1e3, 1)}, **more))

    poses, xy, _ = to.synth(N, 901)
    d_poses, d_xy = torch.from_numpy(poses).cuda(), torch.from_numpy(xy).cuda()
    d_src = torch.arange(N, dtype=torch.int32, device="cuda")
    outs = {"traj": torch.empty((N, 3), dtype=torch.float64, device="cuda"),
            "traj_raw": torch.empty((N, 3), dtype=torch.float64, device="cuda"),
            "resid": torch.empty((N,), dtype=torch.float64, device="cuda"),
            "valid": torch.empty((N,), dtype=torch.int32, device="cuda")}
    nbytes = int(lib.p3d_root_trajectory_workspace(N, 32))
    work = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device="cuda")

    fin, keep = clip_finish_call(N, rng)
    rate("clip_finish", 1, 0, timed_us(fin, reps), SKEL_BYTES["clip_finish"])

    for S in (1, 240):
        cuts = np.sort(rng.choice(np.arange(1, N), size=S - 1, replace=False)) if S > 1 else np.array([], np.int64)
        off = np.concatenate([[0], cuts, [N]]).astype(np.int64)
        d_off = torch.from_numpy(off).cuda()
        L = torch.full((S, 16), 100.0, dtype=torch.float64, device="cuda")
        root = outs["traj_raw"]
        rate("skel_pose_root", S, 0, timed_us(lambda: _p3d.check(lib.p3d_skel_pose(
            p(d_poses), p(d_src), off.ctypes.data, p(d_off), S, N, p(L), None, None, None, p(root), st()), "p3d_skel_pose"),
            reps), 96 * 8 + 4 + 24)

        def call(h, keys):
            ptrs = [p(outs[k]) if k in keys else None for k in ("traj", "traj_raw", "resid", "valid")]
            return lambda: _p3d.check(lib.p3d_root_trajectory(
                p(d_poses), p(d_xy), p(d_src), off.ctypes.data, p(d_off), S, N, to.F, to.CX, to.CY, h, *ptrs, p(work), nbytes,
                st()), "p3d_root_trajectory")

        every = ("traj", "traj_raw", "resid", "valid")
        us_solve = timed_us(call(0, ("traj_raw",)), reps)
        rate("traj_solve_raw_only", S, 0, us_solve, ROW_IN + 4 + 24)
        us0 = 0.0
        for h in (0, 4, 32):
            us = timed_us(call(h, every), reps)
            us0 = us0 or us
            # h > 0: the second launch reads the raw rows and flags again and writes traj -- its share of the time
            rate("traj_all", S, h, us, ROW_IN + 4 + sum(OUT_BYTES.values()), smooth_us=round(us - us0, 2))
        torch.cuda.synchronize()
        assert int(outs["valid"].sum()) == N
        if "--no-oracle" not in sys.argv:
            t0 = time.perf_counter()
            raw, _, ok, _ = to.solve(poses, xy, None, to.F, to.CX, to.CY)
            t1 = time.perf_counter()
            n = min(N, 1 << 14)
            to.smooth(raw[:n], ok[:n], [0, n], 4)
            t2 = time.perf_counter()
            emit({"what": "numpy_oracle", "N": N, "S": S, "solve_us": round(1e6 * (t1 - t0), 1), "smooth_rows": n,
                  "smooth_h4_us": round(1e6 * (t2 - t1), 1)})
            got = outs["traj_raw"].cpu().numpy()
            emit({"what": "gpu_vs_oracle", "N": N, "S": S, "raw_bytes_equal": bool(got.tobytes() == raw.tobytes()),
                  "worst_rel": float((np.abs(got - raw) / np.maximum(1.0, np.abs(raw))).max())})
    del keep


if __name__ == "__main__":
    main()
