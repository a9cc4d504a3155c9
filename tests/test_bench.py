"""
bench.py's line and outputs: a plain run prints the headline without the checks and extra measurements that --full adds, and
--dump-outputs writes what a caller of the timed path receives from its last step -- the same in every run with the same
arguments, and the C oracle's on the same samples.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def run_bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["GF2_DEVICE"] = "0"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--no-settle"] + list(args)
    done = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, text=True)
    assert done.returncode == 0, done.stderr[-3000:]
    lines = [ln for ln in done.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def oracle_inputs():
    import bench
    _, h1, h2 = bench.build_code()
    return bench, h1, h2, bench.P_TOTAL / 3


@pytest.mark.gpu
def test_bench_plain_and_full_lines_and_the_dumped_histograms(tmp_path):
    batch = 1 << 15
    plain = run_bench("--batch-log2", "15", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "plain"))
    assert all(key in plain for key in HEADLINE) and plain["unit"] == "syndromes/s" and plain["higher_is_better"] is True
    assert plain["steps"] == 3 and plain["checks"]["histogram_total"] == 3 * batch
    assert abs(plain["value"] - batch / (plain["ms_per_step"] * 1e-3)) < 1e-6 * plain["value"]
    assert "cpu_baseline" not in plain and "secondary" not in plain and plain["checks"]["oracle_prefix"] is None
    assert "measured_read_peak_GBs" not in plain["roofline"] and plain["roofline"]["frac"] > 0
    full = run_bench("--full", "--no-cpu-baseline", "--no-secondary", "--batch-log2", "15", "--steps", "2", "--warmup", "0",
                     "--dump-outputs", str(tmp_path / "full"))
    assert full["steps"] == 2 and full["checks"]["oracle_prefix"] and full["roofline"]["measured_read_peak_GBs"] > 0
    assert full["roofline"]["mean_call_ms_on_its_stream"] > 0
    # the last step's histograms: independent of the number of steps, and the oracle's over the whole batch
    from oracle import c_oracle
    bench, h1, h2, p = oracle_inputs()
    want = c_oracle.mc(h1, bench.R1, h2, bench.R2, bench.N_QUBITS, bench.SEED, 0, batch, p, p, p, 1)
    for name, hist in zip(("hist_z", "hist_x"), want):
        got = np.load(tmp_path / "plain" / (name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, hist.astype(np.float64))
        assert np.array_equal(np.load(tmp_path / "full" / (name + ".npy")), got)


@pytest.mark.gpu
def test_bench_dumps_a_window_of_the_dense_path_syndromes(tmp_path):
    batch, window = 1 << 16, 1024
    run_bench("--algo", "dense", "--batch-log2", "16", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    from oracle import c_oracle
    bench, h1, h2, p = oracle_inputs()
    first = int(np.random.default_rng(bench.SEED).integers(0, batch - window + 1))      # bench.dump_outputs's window
    ex, ez = c_oracle.sample_errors(bench.N_QUBITS, bench.SEED, first, window, p, p, p)
    for name, h, r, e in (("syndromes_z", h1, bench.R1, ez), ("syndromes_x", h2, bench.R2, ex)):
        got = np.load(tmp_path / (name + ".npy"))
        want = c_oracle.unpack_rows(c_oracle.syndrome_batch(h, r, bench.N_QUBITS, e, window), r)
        assert got.dtype == np.float32 and got.shape == (window, r) and np.array_equal(got, want)
    hz = np.load(tmp_path / "hist_z.npy")
    assert hz.sum() == batch
