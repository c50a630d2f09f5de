"""bench.py's step ranges (--steps / --warmup past the end of the chain), --dump-outputs and what --full adds to a plain run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_segments_run_every_step_once_and_wrap():
    S = 1000
    for first, n in ((0, 1), (10, 200), (5, 995), (990, 20), (2, 1003), (0, 2500), (1500, 7)):
        segs = bench.chain_segments(S, first, n)
        assert sum(k for _, k in segs) == n
        assert all(0 <= t < S and 1 <= k <= t + 1 for t, k in segs)  # what egoego_sample_loop accepts
        ts = [t - j for t, k in segs for j in range(k)]
        assert ts == [S - 1 - i % S for i in range(first, first + n)]
    assert bench.chain_segments(S, 10, 200) == [(989, 200)]  # inside the chain: one call, as before


def test_dump_outputs_writes_float32_and_keeps_the_tree_clean(tmp_path):
    poses = torch.randn(6, 5, 3)
    d = tmp_path / "dump"
    info = bench.dump_outputs(str(d), {"poses": poses})
    got = np.load(d / "poses.npy")
    assert got.dtype == np.float32 and np.array_equal(got, poses.numpy()) and info["poses"]["rows"] == "all"
    assert (d / ".gitignore").read_text() == "*\n"
    # an existing directory is written into as it is
    (tmp_path / "own").mkdir()
    bench.dump_outputs(str(tmp_path / "own"), {"poses": poses})
    assert sorted(os.listdir(tmp_path / "own")) == ["poses.npy"]


def test_dump_outputs_samples_the_same_rows_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 60 * 40)  # 40 of the 100 rows of 60 float32 values
    poses = torch.arange(100 * 60, dtype=torch.float32).view(100, 12, 5)
    for d in ("a", "b"):
        info = bench.dump_outputs(str(tmp_path / d), {"poses": poses})
        assert info["poses"]["shape"] == [40, 12, 5] and info["poses"]["rows"] == "40 of 100 (seeded sample)"
    a, b = np.load(tmp_path / "a" / "poses.npy"), np.load(tmp_path / "b" / "poses.npy")
    assert np.array_equal(a, b)
    rows = a[:, 0, 0].astype(np.int64) // 60
    assert np.all(np.diff(rows) > 0) and np.array_equal(a, poses.numpy()[rows])


def _bench(args, timeout=900):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_bench_times_steps_past_the_chain_and_dumps_the_same_outputs_every_run(tmp_path):
    """--steps larger than the 1000-step chain is timed as asked (the chain starts again), and the poses --dump-outputs writes are
    those of the timed call, the same in two runs of the same command."""
    common = ["--gpus", "1", "--steps", "1003", "--warmup", "2", "--batch", "8", "--no-cpu-baseline", "--no-trained-like"]
    a = _bench(common + ["--dump-outputs", str(tmp_path / "a"), "--dump", str(tmp_path / "a.pt")])
    assert a["steps"] == 1003 and a["ms_per_step"] > 0 and a["output_finite"]
    assert "(steps 997..0, 999..995 timed)" in a["config"]["workload"]
    assert a["dump_outputs"]["files"]["poses"] == {"shape": [8, 120, 198], "dtype": "float32", "rows": "all"}
    got = np.load(tmp_path / "a" / "poses.npy")
    assert got.dtype == np.float32 and np.array_equal(got, torch.load(tmp_path / "a.pt").numpy())
    _bench(common + ["--dump-outputs", str(tmp_path / "b")])
    assert np.array_equal(np.load(tmp_path / "b" / "poses.npy"), got)


@pytest.mark.gpu
def test_plain_run_leaves_out_what_full_measures_and_both_time_the_same_steps(tmp_path):
    """A plain run prints the headline and what it is computed from, and nothing that takes runs of its own: no guarded steps, no
    per-kernel launch times, no trained-like checkpoint, no CPU baseline.  --full adds them (trained_like and cpu_baseline are left out
    here by their own flags) after the same timed call: the same configuration, precision and poses."""
    common = ["--gpus", "1", "--steps", "5", "--warmup", "2", "--batch", "8"]
    plain = _bench(common + ["--dump-outputs", str(tmp_path / "plain")])
    full = _bench(common + ["--full", "--no-cpu-baseline", "--no-trained-like", "--dump-outputs", str(tmp_path / "full")])
    extra = {"ms_per_step_with_checksum_and_guard", "outlier_row_max", "outlier_guard_demoted_after_timed_call", "roofline",
             "roofline_second_kernel"}
    assert not (extra | {"trained_like", "cpu_baseline", "speedup_vs_cpu_baseline"}) & set(plain)
    assert plain["ms_per_step"] > 0 and plain["output_finite"] and plain["value"] == pytest.approx(1e3 / plain["ms_per_step"])
    assert extra <= set(full) and "trained_like" not in full and "cpu_baseline" not in full
    assert full["ms_per_step_with_checksum_and_guard"] > 0 and full["roofline"]["launches"] > 0
    assert full["roofline_second_kernel"]["launches"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype", "precision", "steps", "warmup", "config"):
        assert plain[k] == full[k], k
    assert np.array_equal(np.load(tmp_path / "plain" / "poses.npy"), np.load(tmp_path / "full" / "poses.npy"))
