"""Dev tool: device times of the wide VAE filter (csrc/p3d_vae_wide.h), one JSON line per measurement,
also appended to profiles/vae_wide_probe.jsonl.

At batch 64 and the shape 1360 -> 40 -> 32 -> {24, 24} -> 32 -> 40 -> 48, alternated round by round,
device events around `reps` back-to-back calls, medians reported:

  (a) the training step through the _cat call: [x2d | out_3d | (feature table, idx)];
  (b) the same step through the plain call on a materialised torch.cat + index_select;
  (c) the narrow default step (48 inputs) on the same box;
  (d) the same 1360 step in eager torch: autograd + torch.optim.Adam(eps=1e-7), the three loss terms
      as tests/vae_oracle.py states them -- what a user has without the wide form;

and (e) the forward alone at 2^16 and 2^20 rows with its share of the HBM bound rows * 4 * in bytes.

    python tools/vae_wide_probe.py [--rounds 5] [--reps 200]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-pose-baseline_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from top_vae_3d_pose import models  # noqa: E402

HBM_PEAK = 8.0e12        # bytes / s (MI355X)
FACTORS = (100.0, 0.02, 1.0)
PARENT = (-1, 0, 1, -1, 3, 4, -1, 6, 7, 8, 7, 10, 11, 7, 13, 14)   # tests/vae_oracle.py
WIDE = (1360, (40, 32), 24, (32, 40), 48)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps      # microseconds per call


class EagerVAE(torch.nn.Module):
    """The filter in eager torch (the graph of tests/vae_oracle.py)."""

    def __init__(self, shape):
        super().__init__()
        n_in, enc, lat, dec, out = shape
        dims = [n_in] + list(enc)
        self.enc = torch.nn.ModuleList([torch.nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:])])
        self.mean, self.log_var = torch.nn.Linear(dims[-1], lat), torch.nn.Linear(dims[-1], lat)
        dims = [lat] + list(dec)
        self.dec = torch.nn.ModuleList([torch.nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:])])
        self.out = torch.nn.Linear(dims[-1], out)
        par = torch.tensor([p if p >= 0 else 0 for p in PARENT])
        self.register_buffer("par", par)
        self.register_buffer("has", torch.tensor([1.0 if p >= 0 else 0.0 for p in PARENT]).view(1, 16, 1))

    def bones(self, y):
        j = y.view(-1, 16, 3)
        return j - self.has * j[:, self.par]

    def loss(self, x, t, eps):
        h = x
        for layer in self.enc:
            h = torch.relu(layer(h))
        mean, lv = self.mean(h), self.log_var(h)
        d = eps * torch.exp(0.5 * lv) + mean
        for layer in self.dec:
            d = torch.relu(layer(d))
        y = self.out(d)
        like = ((t - y) ** 2).mean(dim=-1)
        bp, bt = self.bones(y), self.bones(t)
        kcs = (bp @ bp.transpose(1, 2) - bt @ bt.transpose(1, 2)).abs().sum(dim=(1, 2))
        dkl = 0.5 * (torch.exp(lv) + mean ** 2 - 1.0 - lv).sum(dim=-1)
        return FACTORS[0] * like.mean() + FACTORS[1] * kcs.mean() + FACTORS[2] * dkl.mean()


def main():
    arg = lambda k, d: int(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d   # noqa: E731
    rounds, reps = arg("--rounds", 5), arg("--reps", 200)
    assert torch.cuda.is_available(), "the probe needs a GPU"
    out = []
    rng = np.random.default_rng(1)
    dev = torch.device("cuda")
    B = 64
    cat = models.VAE(WIDE[0], WIDE[2], WIDE[1], WIDE[3], max_batch=B, seed=3)
    plain = models.VAE(WIDE[0], WIDE[2], WIDE[1], WIDE[3], max_batch=B, seed=3)
    narrow = models.VAE(48, 24, [40, 32], [32, 40], max_batch=B, seed=3)
    x2 = torch.from_numpy(rng.standard_normal((B, 32)).astype(np.float32)).to(dev)
    x3 = torch.from_numpy(rng.standard_normal((B, 48)).astype(np.float32)).to(dev)
    table = torch.from_numpy((0.1 * rng.standard_normal((100000, 1280))).astype(np.float32)).to(dev)   # 512 MB
    idx = torch.from_numpy(rng.permutation(100000)[:B].astype(np.int64)).to(dev)
    t = torch.from_numpy(rng.standard_normal((B, 48)).astype(np.float32)).to(dev)
    eps = torch.from_numpy(rng.standard_normal((B, 24)).astype(np.float32)).to(dev)
    eager = EagerVAE(WIDE).to(dev)
    opt = torch.optim.Adam(eager.parameters(), lr=1e-4, eps=1e-7)

    def step_plain():
        x = torch.cat([x2, x3, table.index_select(0, idx)], dim=1)
        plain.train_step_device(x, t, FACTORS, 1e-4)

    def step_eager():
        x = torch.cat([x2, x3, table.index_select(0, idx)], dim=1)
        opt.zero_grad(set_to_none=True)
        eager.loss(x, t, eps).backward()
        opt.step()

    cases = {"a_wide_cat_step": lambda: cat.train_step_device([x2, x3, (table, idx)], t, FACTORS, 1e-4),
             "b_wide_plain_step_on_cat_and_index_select": step_plain,
             "c_narrow_default_step": lambda: narrow.train_step_device(x3, t, FACTORS, 1e-4),
             "d_eager_torch_autograd_adam_step": step_eager}
    for fn in cases.values():
        timed(fn, 20)                                # warm every shape
    us = {k: [] for k in cases}
    for _ in range(rounds):                          # alternate the cases round by round
        for k, fn in cases.items():
            us[k].append(round(timed(fn, reps), 3))
    rec = {"what": "vae_wide_step_b64", "shape": "1360-40-32-{24,24}-32-40-48", "reps": reps, "rounds": rounds}
    for k, v in us.items():
        rec[k + "_us"] = v
        rec[k + "_us_median"] = float(np.median(v))
    rec["floor_a_le_d"] = rec["a_wide_cat_step_us_median"] <= rec["d_eager_torch_autograd_adam_step_us_median"]
    out.append(rec)
    for m in (cat, plain, narrow):
        m.close()
    del table
    # (e) the forward alone: HBM-bound on reading x once
    for lg in (16, 20):
        n = 1 << lg
        big = models.VAE(WIDE[0], WIDE[2], WIDE[1], WIDE[3], max_batch=n, seed=3)
        xb = torch.randn((n, WIDE[0]), device=dev)
        eb = torch.randn((n, 24), device=dev)
        fwd = lambda: big.forward_device(xb, eps=eb)   # noqa: E731
        timed(fwd, 3)
        v = [round(timed(fwd, 10), 1) for _ in range(rounds)]
        med = float(np.median(v))
        nbytes = n * 4 * WIDE[0]
        out.append({"what": "vae_wide_fwd_2^%d" % lg, "us": v, "us_median": med, "bytes_x": nbytes,
                    "hbm_bound_us": round(1e6 * nbytes / HBM_PEAK, 1), "GBps": round(nbytes / med / 1e3, 1),
                    "share_of_hbm_bound": round(1e6 * nbytes / HBM_PEAK / med, 3)})
        big.close()
        del xb, eb
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "vae_wide_probe.jsonl"), "a") as f:
        for rec in out:
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
