"""SoftTiedAttentionOverResidues.route() against tests/golden/tied_routes.json (no GPU): the route attend() took for every shape
of a grid, recorded on meta tensors at the commit the file names, before the route choice became a function.  The table is the
authority, quirks included (see route()'s docstring): one character per decision, keyed "dtype/d_msa x heads/B[/switch]", MSA
depths outermost, chain lengths innermost; a key with a switch was recorded with that switch turned off."""
import json
import os

import pytest
import torch

import rosettafold_pytorch_amd as R
from rosettafold_pytorch_amd import ops
from rosettafold_pytorch_amd.runtime import RT

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tied_routes.json")) as fh:
    TABLE = json.load(fh)
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def test_the_table_covers_the_grid():
    assert len(TABLE["parent"]) == 40 and set(TABLE["codes"].values()) == set(R.model.SoftTiedAttentionOverResidues.ROUTES)
    keys = set(TABLE["tables"])
    cfgs = ("384x12", "288x9", "96x3", "768x24", "128x2")
    assert keys >= {f"{dt}/{c}/B{b}" for dt in DTYPES for c in cfgs for b in (1, 2)}
    assert keys >= {f"bf16/{c}/B1/{sw}" for c in cfgs
                    for sw in ("fused_tied", "tied_v2", "tied_fold_w", "tied_long_ragged", "_NO_WREG")}
    assert all(len(v) == len(TABLE["N"]) * len(TABLE["L"]) for v in TABLE["tables"].values())
    assert set("".join(TABLE["tables"].values())) == set(TABLE["codes"])   # every outcome occurs


@pytest.mark.parametrize("key", sorted(TABLE["tables"]))
def test_route_reproduces_the_recorded_table(key, monkeypatch):
    dt, cfg, b, *switch = key.split("/")
    d_msa, heads = (int(v) for v in cfg.split("x"))
    for sw in switch:   # "turned off": a route switch goes False; ops._NO_WREG, which takes a kernel away, goes True
        monkeypatch.setattr(*((ops, sw, True) if sw == "_NO_WREG" else (RT, sw, False)))
    R.set_compute_dtype(DTYPES[dt])
    try:
        m = R.model.SoftTiedAttentionOverResidues(d_msa, heads)
        got = "".join({v: k for k, v in TABLE["codes"].items()}[m.route(int(b[1:]), N, L)] for N in TABLE["N"] for L in TABLE["L"])
    finally:
        R.set_compute_dtype(torch.bfloat16)
    want = TABLE["tables"][key]
    wrong = [(N, L, want[i], got[i]) for i, (N, L) in enumerate((N, L) for N in TABLE["N"] for L in TABLE["L"]) if want[i] != got[i]]
    assert not wrong, (key, "(N, L, recorded, route()):", wrong[:10])
