"""One GraphTransformerBlock with its backward pass (enable_backward) at the initial-coordinate generator's shape of the
benchmark config (B=4, L=256, H=4, d_node=d_edge=32, bf16), on the dense graph and under ops.knn_mask(xyz, aa_idx, 32) of a seeded
random-walk backbone: the forward (no_grad), forward + backward through autograd, the backward's peak extra memory, and the core
kernel pair alone (rf_graph_attention_bwd) next to its byte floor -- one read of e plus one write of de at the fp32 copy rate
DESIGN.md section 3 quotes for these boxes (4.7 TB/s).
One process; every variant is warmed; the variants take turns inside each repeat; device events around --launches calls of one
variant; median and spread (min, max) of the per-call time over --reps repeats.  Prints one JSON object; --out also writes it to a
file (profiles/r10_graph_backward.json), keeping a "kernel_errors" entry the test suite may have put there
(tests/test_graph_backward_gpu.py, RF_GRAPH_BACKWARD_ERRORS).
    python tools/graph_backward_bench.py [--out FILE] [--B 4 --L 256 --H 4 --dn 32 --k 32]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import ops  # noqa: E402

COPY_TBPS = 4.7   # fp32 copy, tools/hbm_probe.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--L", type=int, default=256)
    ap.add_argument("--H", type=int, default=4)
    ap.add_argument("--dn", type=int, default=32)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="run only the variants whose name contains this (for a kernel trace); no file is written")
    a = ap.parse_args()
    assert a.launches >= 20 and a.reps >= 3
    R.set_compute_dtype(torch.bfloat16)
    dev = "cuda"
    B, L, H, dn = a.B, a.L, a.H, a.dn
    HD = H * dn
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    blk = R.GraphTransformerBlock(dn, dn, dn, H, 0.0).to(dev).enable_backward()
    node = torch.randn(B, L, dn, generator=g).to(dev)
    edge = torch.randn(B, L, L, dn, generator=g).to(dev)
    w = torch.randn(B, L, dn, generator=g).to(dev)
    steps = torch.randn(B, L, 3, generator=g)
    ca = torch.cumsum(3.8 * steps / steps.norm(dim=-1, keepdim=True), 1)      # a random walk of 3.8 A steps
    xyz = ca[:, :, None, :] + 0.5 * torch.randn(B, L, 3, 3, generator=g)
    xyz[:, :, 1] = ca
    knn = ops.knn_mask(xyz.to(dev), torch.arange(L).repeat(B, 1).to(dev), a.k)
    q, k, v = (torch.randn(B, L, HD, generator=g).to(ops.h16()).to(dev) for _ in range(3))
    e = torch.randn(B, L, L, HD, generator=g).to(ops.h16()).to(dev)
    gout = torch.randn(B, L, HD, generator=g).to(dev)
    scale = dn ** -0.5
    node_g, edge_g = node.clone().requires_grad_(), edge.clone().requires_grad_()

    def forward(mask):
        with torch.no_grad():
            blk(node, edge, mask)

    def forward_backward(mask):
        for t in [node_g, edge_g] + list(blk.parameters()):
            t.grad = None
        (blk(node_g, edge_g, mask) * w).sum().backward()

    variants = {}
    for tag, mask in (("dense", None), ("knn", knn)):
        variants[f"forward_{tag}"] = lambda m=mask: forward(m)
        variants[f"forward_backward_{tag}"] = lambda m=mask: forward_backward(m)
        variants[f"core_kernels_{tag}"] = lambda m=mask: ops.graph_attention_bwd(q, k, v, e, gout, B, L, H, dn, scale, mask=m)
    if a.only:
        variants = {n: f for n, f in variants.items() if a.only in n}
        for fn in variants.values():
            for _ in range(a.launches):
                fn()
        torch.cuda.synchronize()
        return
    for fn in variants.values():
        for _ in range(5):
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
    # peak extra memory of one forward + backward over what is allocated before it (inputs, weights, cached weight copies)
    peak = {}
    for tag, mask in (("dense", None), ("knn", knn)):
        forward_backward(mask)
        for t in [node_g, edge_g] + list(blk.parameters()):
            t.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        forward_backward(mask)
        torch.cuda.synchronize()
        peak[tag] = torch.cuda.max_memory_allocated() - base
    deg = knn.sum(-1).float()
    e_bytes = e.numel() * e.element_size()
    floor_us = 2 * e_bytes / (COPY_TBPS * 1e12) * 1e6
    res = {"shape": {"B": B, "L": L, "H": H, "d_node": dn, "d_edge": dn}, "dtype": "bfloat16", "device": torch.cuda.get_device_name(0),
           "launches_per_repeat": a.launches, "reps": a.reps, "unit": "us per call (device events around the calls of one repeat)",
           "knn": {"k": a.k, "mean_degree": deg.mean().item(), "min_degree": deg.min().item(), "max_degree": deg.max().item()},
           "e_bytes": e_bytes, "edge_feat_bytes_fp32": edge.numel() * 4,
           "core_byte_floor": {"bytes": 2 * e_bytes, "copy_rate_TBps": COPY_TBPS, "floor_us": floor_us,
                               "what": "one read of e plus one write of de (the second read of e is expected from L2)"},
           "peak_extra_bytes_forward_backward": peak}
    for name, ts in times.items():
        ts = sorted(ts)
        res[name] = {"median_us": ts[len(ts) // 2], "min_us": ts[0], "max_us": ts[-1]}
    for tag in ("dense", "knn"):
        res[f"backward_{tag}_us_by_difference"] = res[f"forward_backward_{tag}"]["median_us"] - res[f"forward_{tag}"]["median_us"]
        # (under the mask only the rows' edges of e are read; de is written whole, zeros included)
        fl = floor_us if tag == "dense" else floor_us * 0.5 * (1.0 + deg.mean().item() / L)
        res[f"core_kernels_{tag}"].update(floor_us=fl, floor_fraction=fl / res[f"core_kernels_{tag}"]["median_us"])
    if a.out and os.path.exists(a.out):
        with open(a.out) as fh:
            old = json.load(fh)
        if "kernel_errors" in old:
            res["kernel_errors"] = old["kernel_errors"]
    print(json.dumps({k_: v_ for k_, v_ in res.items() if k_ != "kernel_errors"}))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
