"""InitialCoordGenerationWithMsaAndPair with its backward pass (enable_backward) at the benchmark config's shape (B=4, N=128,
L=256, d_msa=384, d_pair=288, d_node=d_edge=32, 4 heads, 4 blocks, bf16): the forward (no_grad), forward + backward through
autograd, the backward's peak extra memory, and rf_poswise_bwd alone in the node input's form (collapsed, fused with the
weighted sum: q0 fp32, k = LayerNorm(msa) in the 16-bit type, an fp32 dk) next to the bytes it must move -- k twice, dk once --
and to a bare fp32 copy of a tensor of dk's size measured in the same process (tools/bw_probe.py's reference point; dk is 200 MB
here, under the 256 MB Infinity Cache, so the copy is the hot-loop figure).
One process; every variant is warmed; the variants take turns inside each repeat; device events around --launches calls of one
variant; median and spread (min, max) of the per-call time over --reps repeats.  Prints one JSON object; --out also writes it to a
file (profiles/r12_initial_coord_backward.json), keeping a "kernel_errors" entry the test suite may have put there
(tests/test_poswise_bwd_gpu.py, RF_INITIAL_COORD_BACKWARD_ERRORS).
    python tools/initial_coord_backward_bench.py [--out FILE] [--B 4 --N 128 --L 256 --d_msa 384 --d_pair 288 --dn 32]"""
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
    ap.add_argument("--d_pair", type=int, default=288)
    ap.add_argument("--dn", type=int, default=32)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.launches >= 10 and a.reps >= 3
    R.set_compute_dtype(torch.bfloat16)
    dev = "cuda"
    B, N, L, D, Dp = a.B, a.N, a.L, a.d_msa, a.d_pair
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    mod = R.InitialCoordGenerationWithMsaAndPair(D, Dp, a.dn, a.dn, 4, 4, 0.0).to(dev).enable_backward()
    msa = torch.randn(B, N, L, D, generator=g).to(dev)
    pair = torch.randn(B, L, L, Dp, generator=g).to(dev)
    onehot = torch.nn.functional.one_hot(torch.randint(0, 21, (B, L), generator=g), 21).float().to(dev)
    aa_idx = torch.arange(L).repeat(B, 1).to(dev)
    w = torch.randn(B, L, 3, 3, generator=g).to(dev)
    msa_g, pair_g = msa.clone().requires_grad_(), pair.clone().requires_grad_()
    # rf_poswise_bwd's operands in the node input's form
    k = torch.randn(B, N, L, D, generator=g).to(ops.h16()).to(dev)
    q0 = torch.randn(B, L, D, generator=g).to(dev)
    ds = torch.randn(B, L, D, generator=g).to(dev)
    dk = torch.empty(B, N, L, D, device=dev)
    src = torch.randn(B, N, L, D, device=dev)

    def forward():
        with torch.no_grad():
            mod(msa, pair, onehot, aa_idx)

    def forward_backward():
        for t in [msa_g, pair_g] + list(mod.parameters()):
            t.grad = None
        (mod(msa_g, pair_g, onehot, aa_idx) * w).sum().backward()

    variants = {
        "forward": forward,
        "forward_backward": forward_backward,
        "poswise_bwd": lambda: ops.poswise_bwd(q0, D, k, D, 0, 0, D, B, N, L, 1, D ** -0.5, ds=ds, dk=dk, dk_ld=D, dk_hs=0),
        "copy_fp32_of_dk_size": lambda: dk.copy_(src),
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
    for t in [msa_g, pair_g] + list(mod.parameters()):
        t.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    forward_backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    k_bytes, dk_bytes = k.numel() * k.element_size(), dk.numel() * 4
    res = {"shape": {"B": B, "N": N, "L": L, "d_msa": D, "d_pair": Dp, "d_node": a.dn, "d_edge": a.dn, "heads": 4, "blocks": 4},
           "dtype": "bfloat16", "device": torch.cuda.get_device_name(0), "launches_per_repeat": a.launches, "reps": a.reps,
           "unit": "us per call (device events around the calls of one repeat)",
           "peak_extra_bytes_forward_backward": peak, "dm_fp32_bytes": dk_bytes, "d_msa_fp32_bytes": dk_bytes}
    for name, ts in times.items():
        ts = sorted(ts)
        res[name] = {"median_us": ts[len(ts) // 2], "min_us": ts[0], "max_us": ts[-1]}
    res["backward_us_by_difference"] = res["forward_backward"]["median_us"] - res["forward"]["median_us"]
    moved = 2 * k_bytes + dk_bytes
    copy_rate = 2 * dk_bytes / res["copy_fp32_of_dk_size"]["median_us"] / 1e6      # TB/s, read + write
    res["poswise_bwd"].update(bytes_moved=moved, what="k twice (the second read is expected from L2) plus dk once",
                              rate_TBps=moved / res["poswise_bwd"]["median_us"] / 1e6,
                              hbm_bytes=k_bytes + dk_bytes, hbm_rate_TBps=(k_bytes + dk_bytes) / res["poswise_bwd"]["median_us"] / 1e6)
    res["copy_fp32_of_dk_size"].update(bytes_moved=2 * dk_bytes, rate_TBps=copy_rate)
    res["poswise_bwd"]["fraction_of_copy_rate"] = res["poswise_bwd"]["rate_TBps"] / copy_rate
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
