"""MsaUpdateWithPairAndCoord with its backward pass (enable_backward) at the benchmark config's shape (config 2: B=4, N=128,
L=256, d_msa=384, d_state=32, 4 heads of 32, bf16): the forward (no_grad), forward + backward through autograd, the backward's
peak extra memory, and rf_dist_masked_attention_bwd alone (both kernels: q, k fp32 [B,L,128], d att and the ds map fp32
[B,4,L,L]) next to the bytes it must move -- q and k, d att once from memory, the map written once and read once.  That is
about 8 MB at this shape: the pair is bound by latency, not by bandwidth, and the figure says how far from a byte floor it is,
nothing more.
One process; every variant is warmed; the variants take turns inside each repeat; device events around --launches calls of one
variant; median and spread (min, max) of the per-call time over --reps repeats.  Prints one JSON object; --out also writes it to a
file (profiles/r13_msa_coord_backward.json), keeping a "kernel_errors" entry the test suite may have put there
(tests/test_dist_attention_bwd_gpu.py, RF_MSA_COORD_BACKWARD_ERRORS).
    python tools/msa_coord_backward_bench.py [--out FILE] [--B 4 --N 128 --L 256 --d_msa 384 --d_state 32]"""
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
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--L", type=int, default=256)
    ap.add_argument("--d_msa", type=int, default=384)
    ap.add_argument("--d_state", type=int, default=32)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.launches >= 10 and a.reps >= 3
    R.set_compute_dtype(torch.bfloat16)
    dev = "cuda"
    B, N, L, D, Ds, H, dq = a.B, a.N, a.L, a.d_msa, a.d_state, 4, 32
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    mod = R.MsaUpdateWithPairAndCoord(D, Ds, dq, 4 * D, p_dropout=0.0).to(dev).enable_backward()
    step = torch.randn(B, L, 3, generator=g)
    ca = (3.8 * step / step.norm(dim=-1, keepdim=True)).cumsum(1)   # a random walk of 3.8 A steps: every head masks
    xyz = (ca[:, :, None, :] + torch.randn(B, L, 3, 3, generator=g) * torch.tensor([1.0, 0.0, 1.0])[:, None]).float().to(dev)
    state = torch.randn(B, L, Ds, generator=g).to(dev)
    msa = torch.randn(B, N, L, D, generator=g).to(dev)
    w = torch.randn(B, N, L, D, generator=g).to(dev)
    state_g, msa_g = state.clone().requires_grad_(), msa.clone().requires_grad_()
    # the kernel pair's operands
    q = (torch.randn(B, L, H * dq, generator=g) * dq ** -0.25).to(dev)
    k = (torch.randn(B, L, H * dq, generator=g) * dq ** -0.25).to(dev)
    datt = torch.randn(B, H, L, L, generator=g).to(dev)
    bins = torch.tensor(mod.distance_bins, dtype=torch.float32, device=dev)
    ca_d = xyz[:, :, 1].double()
    in_range = ((ca_d[:, :, None] - ca_d[:, None]).norm(dim=-1)[:, None] < bins.double()[None, :, None, None]).double().mean().item()

    def forward():
        with torch.no_grad():
            mod(xyz, state, msa)

    def forward_backward():
        for t in [state_g, msa_g] + list(mod.parameters()):
            t.grad = None
        (mod(xyz, state_g, msa_g) * w).sum().backward()

    variants = {
        "forward": forward,
        "forward_backward": forward_backward,
        "dist_masked_attention_bwd": lambda: ops.dist_masked_attention_bwd(q, k, xyz, bins, datt, B, L, H, dq),
    }
    for fn in variants.values():
        for _ in range(3):
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
    forward_backward()
    for t in [state_g, msa_g] + list(mod.parameters()):
        t.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    forward_backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    res = {"shape": {"B": B, "N": N, "L": L, "d_msa": D, "d_state": Ds, "heads": H, "d_inner": dq},
           "dtype": "bfloat16", "device": torch.cuda.get_device_name(0), "launches_per_repeat": a.launches, "reps": a.reps,
           "unit": "us per call (device events around the calls of one repeat)",
           "in_range_share_of_pairs": in_range,
           "peak_extra_bytes_forward_backward": peak, "msa_fp32_bytes": msa.numel() * 4}
    for name, ts in times.items():
        ts = sorted(ts)
        res[name] = {"median_us": ts[len(ts) // 2], "min_us": ts[0], "max_us": ts[-1]}
    res["backward_us_by_difference"] = res["forward_backward"]["median_us"] - res["forward"]["median_us"]
    map_bytes = datt.numel() * 4
    moved = 2 * (q.numel() + k.numel()) * 4 + 3 * map_bytes + xyz.numel() * 4
    res["dist_masked_attention_bwd"].update(
        bytes_moved=moved, what="q, k in and dq, dk out, d att read once from memory, the ds map written once and read once, xyz",
        rate_TBps=moved / res["dist_masked_attention_bwd"]["median_us"] / 1e6)
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
