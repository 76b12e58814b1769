"""bench.py's two kinds of run: a plain run does only what the headline needs (its extra figures are null), --full adds the
CPU baseline, the accuracy checks and the latency / MFMA-stream figures.  cfg 1 at a small batch keeps both runs short."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
SMALL = ["--config", "1", "--systems-per-gpu", "64", "--steps", "2", "--warmup", "1"]
EXTRAS = ("max_rel_err_uscat", "sym_vs_lu", "single_system_ms", "cpu_baseline", "marshalling_ms")


def _run(args, timeout):
    p = subprocess.run([sys.executable, BENCH] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_single_system_needs_full():
    p = subprocess.run([sys.executable, BENCH, "--single-system"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 2
    assert "--full" in p.stderr


@pytest.mark.gpu
def test_plain_run_is_headline_only(tmp_path):
    out = _run(SMALL + ["--dump-outputs", str(tmp_path)], timeout=300)
    assert out["unit"] == "systems/s" and out["higher_is_better"] is True and out["dtype"] == "c128"
    assert out["steps"] == 2 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(64 / (out["ms_per_step"] * 1e-3), rel=1e-9)
    for key in EXTRAS:
        assert out[key] is None, key
    assert out["roofline"]["pure_mfma_stream_tflops"] is None
    assert out["config"]["solved_by"] == {"ldlt_systems": 64, "lu_systems": 0}
    re_, im_ = np.load(tmp_path / "density_real.npy"), np.load(tmp_path / "density_imag.npy")
    assert re_.shape == im_.shape == (64, 2, 36)
    assert np.all(np.isfinite(re_)) and np.all(np.isfinite(im_))


@pytest.mark.gpu
def test_full_run_adds_the_checks():
    out = _run(SMALL + ["--full", "--cpu-baseline-systems", "2", "--cpu-baseline-reps", "1", "--sym-vs-lu-systems", "4"], timeout=600)
    assert out["value"] > 0
    assert out["max_rel_err_uscat"] < 1e-10
    assert out["cpu_baseline"]["value"] > 0
    assert out["sym_vs_lu"]["systems"] == 4 and out["sym_vs_lu"]["max_rel_diff_density"] < 1e-10
    assert out["single_system_ms"] > 0
    assert out["roofline"]["pure_mfma_stream_tflops"] > 0
    assert out["marshalling_ms"] is None          # one rank, no process group
