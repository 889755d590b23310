"""bench.py command line: result line fields, --steps, --dump-outputs
reproducibility and --full, on the CPU/TCP path at world 1 (small message)."""
import json
import os
import subprocess
import sys

import numpy as np

from tests.mp import REPO


def _bench(*extra):
    env = dict(os.environ, MLSL_TRANSPORT="tcp", PYTHONPATH=REPO)
    p = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--device", "cpu", *extra],
        env=env, cwd=REPO, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_bench_result_line_and_dump(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    args = ("--mbytes", "1", "--steps", "3", "--warmup", "1")
    ra = _bench(*args, "--dump-outputs", a)
    _bench(*args, "--dump-outputs", b)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype",
                "ms_per_step"):
        assert key in ra, key
    assert ra["steps"] == 3 and ra["warmup"] == 1
    assert ra["ms_per_step"] > 0
    # value is message_bytes / t_step in GB/s (rounded to 3 / 4 places)
    want = (1 << 20) / (ra["ms_per_step"] * 1e-3) / 1e9
    assert abs(ra["value"] - want) <= 0.02 * want + 1e-3
    xa = np.load(os.path.join(a, "allreduce_out.npy"))
    xb = np.load(os.path.join(b, "allreduce_out.npy"))
    assert xa.dtype == np.float32 and xa.shape == (1 << 18,)
    assert np.array_equal(xa, xb)
    # world 1: the allreduce returns the (seeded) message itself
    want_msg = np.random.RandomState(0).randn(1 << 18).astype(np.float32)
    assert np.array_equal(xa, want_msg)


def test_bench_dump_samples_large_output(tmp_path):
    # 32 MiB message = 8 Mi elements > the 4 Mi element dump cap
    d = str(tmp_path / "d")
    _bench("--mbytes", "32", "--steps", "1", "--warmup", "0",
           "--dump-outputs", d)
    x = np.load(os.path.join(d, "allreduce_out.npy"))
    assert x.dtype == np.float32 and x.shape == (1 << 22,)
    # the documented sample, rebuilt here: one seeded position in each of
    # 4 Mi equal strata, both ends forced
    count, m = 1 << 23, 1 << 22
    edges = np.arange(m + 1, dtype=np.int64) * count // m
    width = np.diff(edges)
    frac = np.random.RandomState(12345).random_sample(m)
    idx = edges[:-1] + np.minimum((frac * width).astype(np.int64), width - 1)
    idx[0], idx[-1] = 0, count - 1
    assert (np.diff(idx) > 0).all()  # distinct and sorted
    # world 1: the result is the seeded message, so the dump is msg[idx]
    msg = np.random.RandomState(0).randn(count).astype(np.float32)
    assert np.array_equal(x, msg[idx])


def test_bench_full_flag_runs():
    r = _bench("--mbytes", "1", "--steps", "2", "--warmup", "0", "--full")
    assert r["metric"] == "allreduce_algbw_GBps" and r["steps"] == 2
