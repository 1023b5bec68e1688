"""SoftTiedAttentionOverResidues with its backward pass (enable_backward) at the benchmark config's shape (config 2: B=4, N=128,
L=256, d_msa=384, 12 heads of 32, bf16; return_att=True, a gradient on both outputs): the forward (no_grad), forward + backward
through autograd, the backward's peak extra memory, and the two kernels the backward adds, each alone next to the bytes it
must move and to a bare fp32 copy (rf_axpby) of the same number of bytes on the same device:
  rf_tied_softmax_bwd   logits, dp and g_sym read once, ds written once in fp32, p and ds written once in the 16-bit type;
  rf_scale_rows_bwd     q and dq~ (16-bit) read once, dq (16-bit) written once, w read and dw written (fp32, one per row).
The bytes are a floor, not a model: rf_tied_softmax_bwd reads the logits three times and dp and g_sym twice, the repeats from
cache.  One process; every variant is warmed; the variants take turns inside each repeat; device events around --launches
calls of one variant; median and spread (min, max) of the per-call time over --reps repeats.  Prints one JSON object; --out also
writes it to a file (profiles/r14_tied_backward.json), keeping a "kernel_errors" entry the test suite may have put there
(tests/test_tied_softmax_bwd_gpu.py, RF_TIED_BACKWARD_ERRORS).
    python tools/tied_backward_bench.py [--out FILE] [--B 4 --N 128 --L 256 --d_msa 384 --heads 12]"""
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
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.launches >= 10 and a.reps >= 3
    R.set_compute_dtype(torch.bfloat16)
    dev = "cuda"
    B, N, L, D, H = a.B, a.N, a.L, a.d_msa, a.heads
    dh = D // H
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    mod = R.SoftTiedAttentionOverResidues(D, H, p_dropout=0.0, return_att=True).to(dev).enable_backward()
    x = torch.randn(B, N, L, D, generator=g).to(dev)
    w_o = torch.randn(B, N, L, D, generator=g).to(dev)
    w_a = torch.randn(B, L, L, H, generator=g).to(dev)
    x_g = x.clone().requires_grad_()
    # the kernels' operands
    logits = (torch.randn(B, H, L, L, generator=g) * 3).to(dev)
    dp = torch.randn(B, H, L, L, generator=g).to(dev)
    g_sym = torch.randn(B, L, L, H, generator=g).to(dev)
    rows = B * N * L
    qkp = torch.randn(rows, 3 * D, generator=g).to(torch.bfloat16).to(dev)
    dqt = torch.randn(rows, D, generator=g).to(torch.bfloat16).to(dev)
    wl = torch.rand(rows * H, generator=g).to(dev)
    dqkv = torch.empty(rows, 3 * D, device=dev, dtype=torch.bfloat16)
    softmax_bytes = (logits.numel() + dp.numel() + g_sym.numel() + logits.numel()) * 4 + 2 * B * H * L * ops.tied_ld(L) * 2
    scale_bytes = 3 * rows * D * 2 + 2 * rows * H * 4
    copies = {}
    for name, nbytes in (("softmax", softmax_bytes), ("scale", scale_bytes)):   # a bare fp32 copy: half the bytes in, half out
        n = nbytes // 8
        copies[name] = (torch.randn(n, device=dev), torch.empty(n, device=dev))

    def forward():
        with torch.no_grad():
            mod(x)

    def forward_backward():
        for t in [x_g] + list(mod.parameters()):
            t.grad = None
        out, att = mod(x_g)
        ((out * w_o).sum() + (att * w_a).sum()).backward()

    variants = {
        "forward": forward,
        "forward_backward": forward_backward,
        "tied_softmax_bwd": lambda: ops.tied_softmax_bwd(logits, dp, g_sym, h16_copies=True),
        "tied_softmax_bwd_no_g_sym": lambda: ops.tied_softmax_bwd(logits, dp, None, h16_copies=True),
        "copy_of_tied_softmax_bwd_bytes": lambda: ops.axpby(copies["softmax"][0], 1.0, None, 0.0, copies["softmax"][1]),
        "scale_rows_bwd": lambda: ops.scale_rows_bwd(qkp, 3 * D, dh, dqt, D, dh, wl, dh ** -0.5, rows, H, dh, dx=dqkv, dx_ld=3 * D,
                                                     dx_hs=dh),
        "copy_of_scale_rows_bwd_bytes": lambda: ops.axpby(copies["scale"][0], 1.0, None, 0.0, copies["scale"][1]),
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
    for t in [x_g] + list(mod.parameters()):
        t.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    forward_backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    res = {"shape": {"B": B, "N": N, "L": L, "d_msa": D, "heads": H, "d_head": dh},
           "dtype": "bfloat16", "device": torch.cuda.get_device_name(0), "launches_per_repeat": a.launches, "reps": a.reps,
           "unit": "us per call (device events around the calls of one repeat)",
           "peak_extra_bytes_forward_backward": peak, "msa_fp32_bytes": x.numel() * 4}
    for name, ts in times.items():
        ts = sorted(ts)
        res[name] = {"median_us": ts[len(ts) // 2], "min_us": ts[0], "max_us": ts[-1]}
    res["backward_us_by_difference"] = res["forward_backward"]["median_us"] - res["forward"]["median_us"]
    for name, nbytes, what in (
            ("tied_softmax_bwd", softmax_bytes, "logits, dp and g_sym in, ds out (fp32), p and ds out (16-bit), each once"),
            ("scale_rows_bwd", scale_bytes, "q and dq~ in, dq out (16-bit), w in and dw out (fp32), each once")):
        copy = res[f"copy_of_{name}_bytes"]["median_us"]
        res[name].update(bytes_moved=nbytes, what=what, rate_TBps=nbytes / res[name]["median_us"] / 1e6,
                         copy_rate_TBps=nbytes / copy / 1e6, time_over_copy=res[name]["median_us"] / copy)
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
