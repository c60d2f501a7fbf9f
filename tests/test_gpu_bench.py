"""bench.py as it is run for every change: a plain run times the headline alone, prints one JSON line and, with --dump-outputs,
leaves the film of the timed render behind."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_plain_run_prints_the_headline_alone_and_dumps_the_film(root, tmp_path):
    steps, warmup = 2, 1
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "out")]
    res = subprocess.run(cmd, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == steps and out["warmup"] == warmup and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["counters"]["n_samples"] == 1920 * 1080 * 1024 * steps  # --steps is the number of timed steps
    assert "extra_configs" not in out and "cpu_baseline" not in out  # the secondary legs run with --full only
    assert sorted(os.listdir(tmp_path / "out")) == ["film.npy"]
    film = np.load(tmp_path / "out" / "film.npy")
    assert film.dtype == np.float32 and film.shape == (7, 1080, 1920)
    assert np.isfinite(film).all() and (film[6] == 1024.0 * (steps + warmup)).all()  # every pixel holds every sample of the run
    assert film[:3].sum() > 0
