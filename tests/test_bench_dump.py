"""bench.py --dump-outputs (CPU): what the timed path returned is written as float32 .npy files within the size budget; an
output over its share keeps a sample of rows that is the same from run to run and shared by arrays of the same row count."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _outputs():
    g = torch.Generator().manual_seed(0)
    B, L = 2, 48
    return {"logits_dist": torch.randn(B, L, L, 37, generator=g).bfloat16(), "logits_phi": torch.randn(B, L, L, 19, generator=g),
            "xyz": torch.randn(B, L, 3, 3, generator=g), "plddt": torch.rand(B, L, generator=g)}


def test_small_outputs_are_written_whole(tmp_path):
    arrays = _outputs()
    bench.dump_outputs(arrays, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == sorted(f"{k}.npy" for k in arrays)
    for k, v in arrays.items():
        a = np.load(tmp_path / f"{k}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, v.float().numpy()), k


def test_large_outputs_are_sampled_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 256 << 10)
    arrays = _outputs()
    for d in ("a", "b"):
        bench.dump_outputs(arrays, str(tmp_path / d))
    files = sorted(os.listdir(tmp_path / "a"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_BUDGET_BYTES
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f  # same sample every run
    for k in ("xyz", "plddt"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{k}.npy"), arrays[k].numpy())
    # the sampled rows are rows of the output, and the two logit maps share theirs (the same (b, i, j) pairs)
    dist = arrays["logits_dist"].float().reshape(-1, 37).numpy()
    phi = arrays["logits_phi"].reshape(-1, 19).numpy()
    sd, sp = np.load(tmp_path / "a" / "logits_dist.npy"), np.load(tmp_path / "a" / "logits_phi.npy")
    assert sd.shape[1] == 37 and 0 < sd.shape[0] < dist.shape[0] and sp.shape[0] < phi.shape[0]
    rows_d = [int(np.flatnonzero((dist == r).all(1))[0]) for r in sd]
    rows_p = [int(np.flatnonzero((phi == r).all(1))[0]) for r in sp]
    assert rows_d == sorted(rows_d) and rows_p == sorted(rows_p)
    assert set(rows_d) <= set(rows_p) or set(rows_p) <= set(rows_d)
