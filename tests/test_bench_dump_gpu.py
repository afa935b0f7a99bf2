"""`bench.py --dump-outputs DIR`: two fresh runs with the same arguments write the same arrays, bit for bit (inputs and initial
weights are seeded; every kernel of the timed path is deterministic), in float32 / float64 and within the 64 MB bound."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _run(out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and "roofline" not in d and "cpu_baseline" not in d
    return {f: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_two_runs_dump_identical_outputs(tmp_path):
    a, b = _run(tmp_path / "a"), _run(tmp_path / "b")
    assert set(a) == set(b) and "params.npy" in a and "train_actor_loss.npy" in a
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
