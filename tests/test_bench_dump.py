"""bench.py --dump-outputs: what the last timed step returned (lambda, pcg_iters, pcg_exit) as float .npy files under a size cap, the same
from run to run; and a plain run (no --full) times its steps and nothing else.  CPU: the writer and the argument check.  GPU: two plain
runs with the same arguments dump the same arrays, bit for bit."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

BENCH = os.path.join(ROOT, "bench.py")


def _load(d):
    return {os.path.basename(p)[:-4]: np.load(p) for p in sorted(glob.glob(os.path.join(d, "*.npy")))}


def test_dump_writes_float_arrays_of_the_callers_results(tmp_path):
    lam = np.random.default_rng(1).standard_normal((8, 14 * 4)).astype(np.float32)
    it, ex = np.arange(8, dtype=np.int32) + 3, (np.arange(8) % 2).astype(np.uint8)
    bench.dump_outputs(str(tmp_path), lam, it, ex, 0, 1)
    o = _load(tmp_path)
    assert sorted(o) == ["lambda", "pcg_exit", "pcg_iters"]
    assert o["lambda"].dtype == np.float32 and np.array_equal(o["lambda"], lam)
    assert o["pcg_iters"].dtype == np.float64 and np.array_equal(o["pcg_iters"], it)
    assert o["pcg_exit"].dtype == np.float32 and np.array_equal(o["pcg_exit"], ex)


def test_dump_of_a_large_lambda_is_a_fixed_sample_under_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 4 << 20)
    B = 4096
    lam = np.arange(B * 14 * 32, dtype=np.float32).reshape(B, 14 * 32)          # 7.3 MB: over the cap
    it, ex = np.full(B, 7, np.int32), np.zeros(B, np.uint8)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), lam, it, ex, 0, 1)
        assert sum(os.path.getsize(p) for p in glob.glob(str(tmp_path / sub / "*.npy"))) <= bench.DUMP_LIMIT
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    rows = a["lambda_rows"].astype(np.int64)
    assert 0 < len(rows) < B and np.array_equal(a["lambda"], lam[rows]) and len(a["pcg_iters"]) == B
    assert all(np.array_equal(a[k], b[k]) for k in a)                            # the same rows every run


def test_ranks_write_their_own_lambda_and_rank0_the_gathered_counts(tmp_path):
    lam = np.ones((3, 14 * 2), np.float32)
    for r in (0, 1):
        bench.dump_outputs(str(tmp_path), lam * r, np.arange(6), np.zeros(6, np.uint8), r, 2)
    o = _load(tmp_path)
    assert sorted(o) == ["lambda_rank0", "lambda_rank1", "pcg_exit", "pcg_iters"] and o["pcg_iters"].shape == (6,)
    assert (o["lambda_rank1"] == 1).all() and (o["lambda_rank0"] == 0).all()


def test_zero_steps_is_refused():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0", "--plumbing-only"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice_and_runs_no_side_leg(tmp_path):
    lines = []
    for sub in ("a", "b"):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "96", "--knots", "64",
                            "--dump-outputs", str(tmp_path / sub)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout + r.stderr
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    for o in lines:
        assert o["metric"] == "pcg_iterations_per_sec" and o["steps"] == 3 and o["warmup"] == 1 and o["ms_per_step"] > 0 and o["value"] > 0
        assert "cpu_baseline" not in o and "sustained_value" not in o["config"] and "iiwa_sqp_linear_step_ms" not in o["config"]
        assert o["full_record"] is None
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["lambda", "pcg_exit", "pcg_iters"]
    assert a["lambda"].shape == (96, 14 * 64) and a["lambda"].dtype == np.float32 and np.isfinite(a["lambda"]).all()
    assert ((a["pcg_iters"] >= 1) & (a["pcg_iters"] <= 167)).all() and a["pcg_iters"].mean() == pytest.approx(lines[0]["config"]["mean_pcg_iters"], rel=1e-5)
    assert all(np.array_equal(a[k], b[k]) for k in a)
