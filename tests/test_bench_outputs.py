"""bench.py ``--dump-outputs`` / ``--full`` on the CPU plumbing config: the dump holds what the last timed step left,
as float32 ``.npy`` files within the size budget, and two runs with the same arguments write the same arrays."""

from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--device", "cpu", "--model", "tinystories-17m", "--seq", "32", "--batch", "2", "--warmup", "1"]


def _bench(tmp_path, out, steps, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, "--steps", str(steps), "--dump-outputs", str(out),
           *extra]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}


def test_dump_outputs_repeatable_and_steps_counted(tmp_path):
    res_a, a = _bench(tmp_path, tmp_path / "a", 2)
    res_b, b = _bench(tmp_path, tmp_path / "b", 2, "--full")
    res_c, c = _bench(tmp_path, tmp_path / "c", 3)
    assert {"loss", "grad_norm", "grad_sample", "weight_sample"} <= set(a) and set(a) == set(b) == set(c)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 * 2**20
    assert a["loss"].shape == (1,) and abs(float(a["loss"][0]) - res_a["final_loss"]) < 1e-3
    assert a["grad_sample"].shape == a["weight_sample"].shape and np.isfinite(a["grad_sample"]).all()
    for k in a:  # same arguments (the CPU path is deterministic): the same arrays, with or without --full
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # --steps sets the number of timed steps: one more optimizer step leaves other weights
    assert (res_a["steps"], res_c["steps"]) == (2, 3) and res_a["ms_per_step"] > 0 and res_c["ms_per_step"] > 0
    assert not np.array_equal(a["weight_sample"], c["weight_sample"])
