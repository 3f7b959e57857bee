"""bench.py --dump-outputs on the GPU: a plain run (no --full) of a small
workload writes the last timed step's sorted records at its sampled
positions, and they are the oracle's stable sort of the reference input."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_sorted_records(lsb_built, oracle_mod, tmp_path):
    n = 100_003  # odd, more than one 4096-record block, blocks overlap the last one
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--n-per-gpu", str(n), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 2 and len(line["step_ms"]) == 2 and line["ms_per_step"] > 0
    # a plain run: nothing but the headline
    assert line["verified"] is None and line["cpu_baseline"] is None
    assert (line["roofline"] or {}).get("traffic") is None
    assert not [k for k in line if k.startswith(("hybrid_", "x16_"))]

    want = oracle_mod.stable_sort(oracle_mod.generate(n, 1))
    arrs = {name: np.load(out / f"rank0_{name}.npy") for name in ("pos", "key_hi", "key_lo", "val")}
    assert sorted(os.listdir(out)) == sorted(f"rank0_{name}.npy" for name in arrs)
    assert all(a.dtype == np.float64 for a in arrs.values())
    pos = arrs["pos"].astype(np.int64)
    assert pos.size >= 2 * 4096 and pos.min() == 0 and pos.max() == n - 1
    key = (arrs["key_hi"].astype(np.uint64) << np.uint64(32)) | arrs["key_lo"].astype(np.uint64)
    assert np.array_equal(key, want["key"][pos])
    assert np.array_equal(arrs["val"].astype(np.uint64), want["val"][pos])
