"""bench.py's plain run, --dump-outputs and --full (one small workload: B=1, 128x64, 2 timed steps).

A plain run prints the headline figure only; --dump-outputs DIR writes what the last timed step
left its caller as float32 .npy files (identical from run to run: seeded inputs and parameters);
--full adds the roofline probe and the CPU baseline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "1", "--height", "64", "--width", "128"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _run(args):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    return subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True,
                          timeout=240)


def _line(r):
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("bad", [["--steps", "0"], ["--steps", "-3"], ["--warmup", "-1"]])
def test_bad_step_counts_refused(bad):
    r = _run(["--gpus", "1"] + bad)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr
    assert r.stdout.strip() == ""


@pytest.mark.gpu
def test_plain_run_dumps_last_step(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    out = _line(_run(SMALL + ["--dump-outputs", a]))
    for k in HEADLINE:
        assert k in out, k
    assert out["steps"] == 2 and out["warmup"] == 1
    assert out["ms_per_step"] > 0
    # images/s and ms per step are the same measurement (both rounded in the line)
    assert out["value"] == pytest.approx(1 * 1e3 / out["ms_per_step"], rel=1e-3)
    for k in ("roofline", "roofline_photometric", "conv_other", "cpu_baseline"):
        assert k not in out, k
    names = sorted(os.listdir(a))
    assert names == ["disp_0.npy", "disp_1.npy", "disp_2.npy", "disp_3.npy", "grad.npy", "loss.npy",
                     "params.npy", "pose.npy"]
    arrs = {n: np.load(os.path.join(a, n)) for n in names}
    assert sum(x.nbytes for x in arrs.values()) <= 64 * 2 ** 20
    for n, x in arrs.items():
        assert x.dtype == np.float32 and x.size > 0 and np.isfinite(x).all(), n
    assert arrs["loss.npy"].shape == (1,) and float(arrs["loss.npy"][0]) == np.float32(out["loss"])
    assert arrs["pose.npy"].shape == (2, 6)
    assert [arrs[f"disp_{i}.npy"].shape for i in range(4)] == [(1, 1, 8, 16), (1, 1, 16, 32),
                                                               (1, 1, 32, 64), (1, 1, 64, 128)]
    assert arrs["params.npy"].shape == arrs["grad.npy"].shape == (2 ** 21,)
    assert np.abs(arrs["grad.npy"]).max() > 0
    # the same arguments give the same inputs and, the step being deterministic, the same outputs
    _line(_run(SMALL + ["--dump-outputs", b]))
    for n in names:
        assert np.array_equal(arrs[n], np.load(os.path.join(b, n))), n


@pytest.mark.gpu
def test_full_run_adds_probe():
    # (the CPU baseline of --full takes >= 14 oracle steps: left to a --full run of the bench)
    out = _line(_run(SMALL + ["--full", "--no-cpu-baseline", "--probe-steps", "2"]))
    for k in HEADLINE:
        assert k in out, k
    assert out["roofline"]["launches"] > 0 and out["roofline"]["kernel_ms_per_step"] > 0
    assert out["roofline_photometric"]["launches"] > 0
    assert out["conv_other"]["launches"] > 0
    assert "cpu_baseline" not in out
