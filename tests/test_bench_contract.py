"""The driver's contract with bench.py: ONE JSON line on stdout with the agreed keys, run here on the small config C2 -- a
plain run (the headline fields and nothing else) and a --full run with every side block that needs minutes switched off
(the side blocks that remain -- the roofline, the assembly, the seam, the launch counts -- are checked for their shape)."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_line(*args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", "C2", *args]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_prints_the_headline_and_nothing_that_takes_runs_of_its_own(tmp_path):
    d = _bench_line("--dump-outputs", str(tmp_path))
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "preconditioner", "iterations", "rel_residual", "setup_seconds", "dump_outputs"):
        assert key in d, key
    assert d["metric"] == "CG solves/s" and d["unit"] == "solves/s" and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["dtype"] == "f64" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert d["iterations"] > 5 and d["rel_residual"] <= 1.1e-12 and d["preconditioner"]["kind"] == "amg"
    for key in ("roofline", "assembly", "value_with_assembly", "seam", "c5", "small", "rank_proxy", "dist_one_rank", "cpu_baseline"):
        assert key not in d, key
    assert "launches" not in d["preconditioner"]
    got = {k: np.load(tmp_path / f"{k}.npy") for k in d["dump_outputs"]["arrays"]}
    assert sorted(got) == ["abs_residual", "iterations", "rel_residual", "x", "x_index"]
    n = d["config"]["n_unknowns"]
    assert got["x"].shape == (n,) and np.isfinite(got["x"]).all() and int(got["iterations"]) == d["iterations"]


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_agreed_keys(tmp_path):
    d = _bench_line("--full", "--no-cpu-baseline", "--no-c5", "--no-rank-proxy", "--no-small", "--no-dist-one-rank",
                    "--dump-outputs", str(tmp_path))
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline"):
        assert key in d, key
    assert d["metric"] == "CG solves/s" and d["unit"] == "solves/s" and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["dtype"] == "f64" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6 * 1e3               # value = steps / elapsed, ms_per_step = elapsed / steps
    r = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in r, key
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert 0.05 < r["frac"] < 1.0                                                # a measured rate, below the peak
    assert d["iterations"] > 5 and d["rel_residual"] <= 1.1e-12 and d["preconditioner"]["kind"] == "amg"
    assert d["assembly"]["ms"] > 0 and len(d["assembly"]["ms_each"]) == 10 and d["seam"]["ms_per_solve"] > d["ms_per_step"]
    assert d["preconditioner"]["launches"]["per_setup"] > 50
    # --dump-outputs: the whole x of C2 (1 M unknowns, below the sampling limit) and the residuals of the last timed step
    assert sorted(d["dump_outputs"]["arrays"]) == ["abs_residual", "iterations", "rel_residual", "x", "x_index"]
    got = {k: np.load(tmp_path / f"{k}.npy") for k in d["dump_outputs"]["arrays"]}
    assert all(a.dtype == np.float64 for a in got.values())
    n = d["config"]["n_unknowns"]
    assert got["x"].shape == (n,) and np.array_equal(got["x_index"], np.arange(n)) and np.isfinite(got["x"]).all()
    assert int(got["iterations"]) == d["iterations"] and float(got["rel_residual"]) == d["rel_residual"]


def test_dump_outputs_samples_a_long_solution_at_fixed_positions(tmp_path):
    """Above bench.DUMP_SAMPLE entries x is written at the same seeded, ascending positions in every run, well inside 64 MB."""
    import bench
    n = bench.DUMP_SAMPLE + 12345
    x = np.arange(n, dtype=np.float64) * 0.5
    res = types.SimpleNamespace(iterations=17, rel_residual=9e-13, abs_residual=2e-10)
    names = bench.dump_outputs(str(tmp_path / "a"), x, res)
    bench.dump_outputs(str(tmp_path / "b"), x, res)
    for k in names:
        assert np.array_equal(np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy"))
    idx = np.load(tmp_path / "a" / "x_index.npy")
    assert len(idx) == bench.DUMP_SAMPLE and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert np.array_equal(np.load(tmp_path / "a" / "x.npy"), x[idx.astype(np.int64)])
    assert float(np.load(tmp_path / "a" / "iterations.npy")) == 17
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 << 20
