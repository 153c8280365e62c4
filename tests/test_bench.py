"""bench.py's command line: a plain run prints the headline line only (the evidence blocks come with --full), --steps sets the
number of timed steps, and --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run_bench(*args, timeout=300):
    r = subprocess.run([sys.executable, BENCH, *args], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=timeout)
    return r


def test_bench_options_parse_without_a_gpu():
    r = run_bench("--help", timeout=60)
    assert r.returncode == 0, r.stderr
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in r.stdout, opt
    r = run_bench("--steps", "0", timeout=60)
    assert r.returncode == 2 and "--steps" in r.stderr, r.stderr


def headline(r):
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-3000:]
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["unit"] == "images/sec" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert out["ms_per_step"] > 0 and out["value"] > 0
    return out


@pytest.mark.gpu
@pytest.mark.timeout(400)
def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    d = tmp_path / "out"
    out = headline(run_bench("--steps", "3", "--warmup", "1", "--batch", "2", "--size", "64", "--dump-outputs", str(d)))
    assert out["steps"] == 3 and out["warmup"] == 1
    assert abs(out["value"] - 2 * 3 / (3 * out["ms_per_step"] * 1e-3)) < 0.01 * out["value"]
    for k in ("roofline", "cpu_baseline", "levels", "other_configs", "clock", "launch_census"):
        assert out[k] is None, k                 # evidence blocks belong to --full
    assert out["kernels"] == {}
    a = {n: np.load(d / f"{n}.npy") for n in ("loss", "logits", "params", "grads", "buffers")}
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert a["loss"].dtype == np.float64 and a["loss"].shape == ()
    assert abs(float(a["loss"]) - out["config"]["final_loss"]) < 1e-5
    assert a["logits"].shape == (2, 3, 64, 64)
    assert a["params"].shape == a["grads"].shape and a["params"].size > 0 and a["buffers"].size > 0
    for n, x in a.items():
        assert x.dtype in (np.float32, np.float64), n
        assert np.isfinite(x).all(), n
    assert np.abs(a["grads"]).max() > 0


@pytest.mark.gpu
@pytest.mark.timeout(400)
def test_full_run_adds_the_evidence_blocks():
    out = headline(run_bench("--steps", "2", "--warmup", "1", "--batch", "2", "--size", "64", "--full", "--no-cpu-baseline"))
    assert out["steps"] == 2
    assert out["roofline"] is not None and out["kernels"]
    assert out["levels"] and out["clock"] is not None and out["launch_census"] is not None
