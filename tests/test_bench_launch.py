"""bench.py's N-rank entry point (host logic, no GPU): `--gpus N` outside a launcher starts
N ranks under torch.distributed.run itself; inside a launcher the rank count must match."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run(args, env=None):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, env=e, timeout=120)


def test_gpus_n_starts_n_ranks():
    r = run(["--gpus", "4", "--steps", "20", "--warmup", "5", "--launch-dry-run"])
    assert r.returncode == 0, r.stderr
    cmd = json.loads(r.stdout.strip().splitlines()[-1])["launch"]
    i = cmd.index("--nproc-per-node")
    assert cmd[i + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert cmd[-6:] == ["--gpus", "4", "--steps", "20", "--warmup", "5"]


def test_rank_count_mismatch_fails():
    r = run(["--gpus", "8"], env={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "--gpus 8 but the job has 2 rank(s)" in r.stderr


def test_full_is_off_by_default():
    sys.path.insert(0, ROOT)
    import bench
    ap = bench.build_arg_parser()
    assert ap.parse_args([]).full is False and ap.parse_args([]).dump_outputs is None
    a = ap.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3", "--full", "--dump-outputs", "d"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (True, "d", 7, 3)


def test_dump_outputs_files(tmp_path, monkeypatch):
    """--dump-outputs: float32/float64 .npy files; an array over its share is cut to the same
    seeded sample of its leading axis in every run; only the first call of a run writes."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 4000)           # two arrays: 2000 bytes each
    rng = np.random.default_rng(1)
    big = rng.standard_normal((100, 10))                     # 8000 bytes: 25 of its 100 rows fit
    small = rng.standard_normal((3, 4)).astype(np.float32)
    ints = np.arange(6).reshape(2, 3)
    got = []
    for sub in ("a", "b"):
        args = bench.build_arg_parser().parse_args(["--dump-outputs", str(tmp_path / sub)])
        bench.dump_outputs(args, 0, big=big, small=small)
        assert args.dump_outputs is None
        bench.dump_outputs(args, 0, big=big[:1], small=small)    # a later measurement: no effect
        got.append({f: np.load(tmp_path / sub / f) for f in sorted(os.listdir(tmp_path / sub))})
    a, b = got
    assert sorted(a) == ["big.npy", "small.npy"]
    assert a["big.npy"].shape == (25, 10) and a["big.npy"].dtype == np.float64
    assert np.array_equal(a["big.npy"], b["big.npy"])
    rows = [int(np.flatnonzero((big == r).all(1))[0]) for r in a["big.npy"]]
    assert rows == sorted(set(rows))                          # distinct rows of the array, in order
    assert a["small.npy"].dtype == np.float32 and np.array_equal(a["small.npy"], small)
    args = bench.build_arg_parser().parse_args(["--dump-outputs", str(tmp_path / "c")])
    bench.dump_outputs(args, 1, ints=ints)                    # not rank 0: nothing written
    assert not (tmp_path / "c").exists()
    args = bench.build_arg_parser().parse_args(["--dump-outputs", str(tmp_path / "c")])
    bench.dump_outputs(args, 0, ints=ints)
    assert np.load(tmp_path / "c" / "ints.npy").dtype == np.float64
