"""bench.py on the GPU box: a plain run prints the headline line and nothing else it does not need (no roofline, parity or
cpu_baseline leg), --dump-outputs still writes the last step's results; --full adds the legs.  Config 5 (the structure
module alone) keeps both runs short; it has a roofline leg and no parity / cpu legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric": str, "value": float, "unit": str, "n_gpus": int, "steps": int, "warmup": int, "ms_per_step": float,
            "higher_is_better": bool, "dtype": str}
LEGS = ("roofline", "parity", "cpu_baseline")


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "5", "--steps", "2",
                        "--warmup", "1", *args], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for k, t in HEADLINE.items():
        assert isinstance(d[k], t), (k, d.get(k))
    assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    return d


def test_plain_run_is_the_headline_only(tmp_path):
    d = _bench("--dump-outputs", str(tmp_path))
    assert not [k for k in LEGS if k in d], sorted(d)
    assert sorted(os.listdir(tmp_path)) == ["state.npy", "xyz.npy"]
    for f in ("state.npy", "xyz.npy"):
        a = np.load(tmp_path / f)
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all(), f


def test_full_run_adds_the_roofline():
    d = _bench("--full")
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["launches"] > 0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert "parity" not in d and "cpu_baseline" not in d  # config 2 only
