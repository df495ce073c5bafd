"""The driver's entry points: smoke() on the GPU, and the bench's JSON contract on a tiny run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_smoke_runs():
    import __graft_entry__ as g
    g.smoke()


@pytest.mark.gpu
def test_bench_emits_one_contract_line():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1",
                          "--directions", "64", "--horizon", "50", "--cpu-seconds", "0.5", "--full"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["dtype"] == "f64" and d["vs_baseline"] is None
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(d["roofline"])
    assert set(("value", "unit", "cores", "kind", "sample")) <= set(d["cpu_baseline"])
    assert d["value"] > 0 and "workload" in d["config"]


@pytest.mark.gpu
def test_plain_bench_times_only_the_steps_and_dumps_what_they_computed(tmp_path):
    """Without --full the line carries the headline only; --dump-outputs writes the last timed step's results, the
    same bit for bit in two runs with the same arguments (seeded inputs, deterministic kernels)."""
    dumps = []
    for run in range(2):
        out_dir = tmp_path / f"run{run}"
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "1",
                              "--directions", "64", "--horizon", "50", "--dump-outputs", str(out_dir)],
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "config"):
            assert key in d, key
        assert d["steps"] == 5 and d["ms_per_step"] > 0 and d["value"] > 0
        assert abs(d["value"] - 2 * 64 * 50 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
        assert not {"roofline", "aux", "cpu_baseline"} & set(d)
        dumps.append({p.stem: np.load(p) for p in out_dir.glob("*.npy")})
    a, b = dumps
    assert set(a) == {"returns", "policy", "mean", "covariance"}
    assert a["returns"].shape == (128,) and a["policy"].shape == (2, 8) and a["mean"].shape == (8,)
    assert a["covariance"].shape == (8, 8)
    for name in a:
        assert a[name].dtype == np.float64 and np.isfinite(a[name]).all(), name
        assert np.array_equal(a[name], b[name]), name
    assert np.abs(a["policy"]).max() > 0          # the timed steps did update the policy
