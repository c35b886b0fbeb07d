"""A plain `bench.py` run on a small C3 queue: it times --steps steps, prints
the line with ms_per_step and nothing of what --full adds, and --dump-outputs
writes the last timed step's results (a row per pair, queue order) and the
constraints gathered from them; the same arguments write the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

NODES, SLICE, STEPS = 48, 5, 3
# Chunks of 4 submaps over slices of 5: chunks straddle the steps.
SMALL = ["--gpus", "1", "--c3-nodes", str(NODES), "--c3-submaps", "12", "--c3-slice", str(SLICE),
         "--steps", str(STEPS), "--warmup", "1"]


def _run(tmp_path, name):
    out = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL,
                        "--dump-outputs", str(out), "--dump-records", str(tmp_path / f"{name}.npz")],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [line for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), out


def test_plain_run_is_lean_and_dumps_last_step(tmp_path):
    j, out = _run(tmp_path, "a")
    assert j["steps"] == STEPS and j["config"]["queue_pairs_timed"] == STEPS * SLICE * NODES
    assert j["ms_per_step"] > 0 and j["unit"] == "pairs/s" and j["higher_is_better"] is True
    assert abs(j["value"] - STEPS * SLICE * NODES / (j["ms_per_step"] * 1e-3 * STEPS)) < 1e-6 * j["value"]
    for key in ("cpu_baseline", "parity_sample", "work_ratio", "c2", "c2_strict", "rt2d", "rt3d",
                "fast3d"):
        assert key not in j, key
    assert sorted(os.listdir(out)) == ["c3_records.npy", "c3_results.npy"]
    res, rec = np.load(out / "c3_results.npy"), np.load(out / "c3_records.npy")
    assert res.dtype == np.float64 and rec.dtype == np.float64
    assert res.shape == (SLICE * NODES, 6)
    assert set(np.unique(res[:, 0])) <= {0.0, 1.0}  # CSM_OK, CSM_NO_MATCH
    # The records are the step's accepted pairs, and the tail of the run's.
    first = (STEPS - 1) * SLICE * NODES
    ok = np.nonzero(res[:, 0] == 0)[0]
    assert len(ok) > 0
    assert np.array_equal(rec[:, 0], first + ok)
    assert np.array_equal(rec[:, 5:8], res[ok, 2:5]) and np.array_equal(rec[:, 8], res[ok, 1])
    whole = np.load(tmp_path / "a.npz")["c3"]
    assert len(whole) == j["accepted_constraints"]
    assert np.array_equal(whole[whole[:, 0] >= first], rec)
    # The same arguments: the same inputs, so the same outputs.
    _, again = _run(tmp_path, "b")
    for name in ("c3_results.npy", "c3_records.npy"):
        assert np.array_equal(np.load(out / name), np.load(again / name)), name
