"""bench.py's plain run on the GPU: only the headline leg, and --dump-outputs writes what the timed path
returned for its last call (the chain state after the last timed step and that call's per-step outputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_headline_only_and_dumps_the_last_call(tmp_path):
    out = tmp_path / "out"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 7 and line["warmup"] == 3 and line["n_gpus"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["dtype"] == "f64"
    assert line["roofline"]["calls"] == 1                      # 7 steps: one timed call
    assert not any(line["recoveries"].values()), line["recoveries"]
    # nothing beside the headline ran
    assert line["full"] is False and line["diagnostics"] is None and line["ranks"]["predicted"] is None
    for leg in ("cpu_baseline", "chain_batched", "mlp", "plantvillage_sgld"):
        assert line[leg] is None, leg
    shapes = {"weights": (784, 10), "bias": (10,), "accept_prob": (7,), "accepted": (7,), "log_likelihood": (7,),
              "energies": (7, 2), "path_length": (7,)}
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in shapes)
    a = {n: np.load(out / (n + ".npy")) for n in shapes}
    for n, shp in shapes.items():
        assert a[n].dtype == np.float64 and a[n].shape == shp, n
        assert np.isfinite(a[n]).all(), n
    # the dumped call is the timed one: its path lengths give the line's leapfrog count
    assert float(np.maximum(0.0, a["path_length"] - 1).sum()) == line["leapfrogs"]
    assert set(np.unique(a["accepted"])) <= {0.0, 1.0}
    assert np.all((a["accept_prob"] >= 0) & (a["accept_prob"] <= 1))
    assert np.abs(a["weights"]).max() > 0                      # the chain left its zero start
