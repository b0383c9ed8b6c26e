"""A plain `bench.py --gpus 1 --steps K --warmup W` run: the headline alone, K timed steps, and with
--dump-outputs the arrays the timed path wrote, which must be the oracle's eval forward of the
benchmark's own seeded inputs (tolerance as tests/test_gpu_serve.py: |d| <= 2e-5 + 2e-5|ref|, fp32
MFMA chain vs the fp64 oracle).  One benchmark process serves every test of this module."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from oracle import ref_mlp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 20, 5


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bench_out"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--dump-outputs", d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, "stdout carries exactly the one JSON line"
    return json.loads(lines[0]), d


def test_plain_line_is_the_headline_alone(plain_run):
    line, _ = plain_run
    assert line["metric"] == "poses/sec at batch 64 (H3.6M 16-joint)"
    assert line["unit"] == "poses/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    # value and ms_per_step are the same timed region: 64 poses per step (each rounded as printed)
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(64 / (line["ms_per_step"] * 1e-3), rel=2e-3)
    # nothing that --full adds
    assert line["roofline"] is None and line["cpu_baseline"] is None
    for k in ("latency_b64", "stream_chain", "single_stream", "train", "eval_sweep", "api_step", "data_pipeline",
              "stress", "cfg1"):
        assert k not in line


def test_dumped_outputs_match_oracle(plain_run):
    _, d = plain_run
    assert os.listdir(d) == ["y.npy"]
    y = np.load(os.path.join(d, "y.npy"))
    assert y.dtype == np.float32 and y.shape == (STEPS, 64, 48)
    import bench
    model, _ = bench.make_model(data_parallel=False, max_batch=64)
    w = model.get_weights()
    model.close()
    cfg = ref_mlp.Cfg(linear_size=bench.L, num_layers=bench.NBLK, residual=True, batch_norm=True)
    st = ref_mlp.State(cfg=cfg, params={k: v for k, v in w.items() if "/moving_" not in k},
                       moving={k: v for k, v in w.items() if "/moving_" in k})
    x = np.random.default_rng(100).standard_normal((STEPS, 64, 32)).astype(np.float32)   # bench_serve's draw, rank 0
    ref, _ = ref_mlp.forward(st, x.reshape(-1, 32), False, 1.0, 0, 0, 0)
    err = np.abs(y.reshape(-1, 48).astype(np.float64) - ref)
    tol = 2e-5 + 2e-5 * np.abs(ref)
    assert np.all(err <= tol), "max err %.3g" % err.max()
