"""GraphTransformer attention core at the initial-coordinate generator's shape of the benchmark config (B=4, L=256, H=4, d=32,
16-bit operands), three ways: the dense entry point (rf_graph_attention), the masked one (rf_graph_attention_masked) under an
all-ones mask, and the masked one under ops.knn_mask(xyz, aa_idx, 32) of a seeded random-walk backbone.
One process; every variant is warmed; the variants take turns inside each repeat; device events around --launches launches of one
variant; median and spread (min, max) of the per-launch time over --reps repeats.  Prints one JSON object; --out also writes it
to a file (profiles/*graph_attention_masked.json).
    python tools/graph_attention_bench.py [--out FILE] [--B 4 --L 256 --H 4 --d 32 --k 32]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--L", type=int, default=256)
    ap.add_argument("--H", type=int, default=4)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.launches >= 200 and a.reps >= 1
    R.set_compute_dtype(torch.bfloat16)
    dev = "cuda"
    B, L, H, d = a.B, a.L, a.H, a.d
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(B, L, H * d, generator=g).to(ops.h16()).to(dev) for _ in range(3))
    e = torch.randn(B, L, L, H * d, generator=g).to(ops.h16()).to(dev)
    steps = torch.randn(B, L, 3, generator=g)
    ca = torch.cumsum(3.8 * steps / steps.norm(dim=-1, keepdim=True), 1)      # a random walk of 3.8 A steps
    xyz = ca[:, :, None, :] + 0.5 * torch.randn(B, L, 3, 3, generator=g)
    xyz[:, :, 1] = ca
    aa_idx = torch.arange(L).repeat(B, 1)
    knn = ops.knn_mask(xyz.to(dev), aa_idx.to(dev), a.k)
    ones = torch.ones(B, L, L, device=dev, dtype=torch.uint8)
    out = torch.empty(B, L, H * d, device=dev)
    scale = d ** -0.5
    variants = {"dense": lambda: ops.graph_attention(q, k, v, e, out, B, L, H, d, scale),
                "masked_all_ones": lambda: ops.graph_attention(q, k, v, e, out, B, L, H, d, scale, mask=ones),
                "masked_knn": lambda: ops.graph_attention(q, k, v, e, out, B, L, H, d, scale, mask=knn)}
    for fn in variants.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(a.reps):
        for name, fn in variants.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.launches):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(1e3 * t0.elapsed_time(t1) / a.launches)
    deg = knn.sum(-1).float()
    res = {"shape": {"B": B, "L": L, "H": H, "d": d}, "dtype": "bfloat16", "device": torch.cuda.get_device_name(0),
           "launches_per_repeat": a.launches, "reps": a.reps, "unit": "us per launch (device events around the launches of one repeat)",
           "knn": {"k": a.k, "mean_degree": deg.mean().item(), "min_degree": deg.min().item(), "max_degree": deg.max().item()},
           "e_bytes": e.numel() * e.element_size()}
    for name, ts in times.items():
        ts = sorted(ts)
        res[name] = {"median_us": ts[len(ts) // 2], "min_us": ts[0], "max_us": ts[-1]}
    res["masked_all_ones_over_dense"] = res["masked_all_ones"]["median_us"] / res["dense"]["median_us"]
    res["masked_knn_over_dense"] = res["masked_knn"]["median_us"] / res["dense"]["median_us"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
