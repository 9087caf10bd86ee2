"""bench.py --dump-outputs writes what the timed path computed in its last step; a plain run (no --full) reports the headline figure only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_stays_within_its_budget_by_a_seeded_sample(tmp_path):
    big = np.arange(4000 * 41 * 60, dtype=np.float64).reshape(4000, 41, 60)  # 80 MB in all
    arrays = {"factor": big, "x": big[:, 0, :40]}
    bench.dump_outputs(str(tmp_path / "a"), arrays, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), arrays, 0, 1)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["factor.npy", "problem_index.npy", "x.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_BYTES
    idx = np.load(tmp_path / "a" / "problem_index.npy").astype(np.int64)
    assert 0 < len(idx) < 4000 and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "factor.npy"), big[idx])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "x.npy"), big[idx, 0, :40])
    for f in files:  # the same sample every time
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_dump_of_a_small_batch_is_whole_and_float(tmp_path):
    bench.dump_outputs(str(tmp_path), {"x": np.ones((8, 3)), "ranks": np.full((8, 5), 12, np.uint32)}, 1, 2)
    assert sorted(os.listdir(tmp_path)) == ["ranks_rank1.npy", "x_rank1.npy"]
    r = np.load(tmp_path / "ranks_rank1.npy")
    assert r.dtype == np.float64 and r.shape == (8, 5) and (r == 12).all()


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(hip, oracle, tmp_path):
    """three timed steps over the four resident batches: the files hold resident batch 2, not batch 0 that the guard re-runs afterwards"""
    from lexls_amd import problems as P
    batch, steps = 512, 3
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", str(batch),
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0
    assert not {"cpu_baseline", "factor_kept", "config1_large", "config4_lsi"} & set(line)  # those belong to --full
    j = (steps - 1) % 4
    lod = P.lse_batch_fast(bench.SEED0 + j * batch + 7919 * j, batch, bench.NVAR, bench.DIMS)
    ref = oracle.lse_run(lod, bench.DIMS, bench.NVAR)
    got = {k: np.load(tmp_path / f"{k}.npy") for k in ("x", "ranks", "column_permutations")}
    assert all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got["ranks"], ref["rank"])
    np.testing.assert_array_equal(got["column_permutations"], ref["perm"])
    assert np.abs(got["x"] - ref["x"]).max() <= 1e-10
