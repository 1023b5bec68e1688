"""MsaUpdateWithPair with its backward pass (enable_backward) at the benchmark config's shape (config 2: B=4, N=128, L=256,
d_msa=384, d_pair=288, 4 layers of 4 heads, bf16): the forward (no_grad), forward + backward through autograd, the backward's
peak extra memory, and the two kernels the backward adds, each next to the bytes it must move and to a bare rf_axpby copy that
moves as many bytes (read + written) in the same run:
  rf_pair_softmax_bwd    logits and d att read once, dz written once in fp32 and once in the 16-bit type;
  rf_sym_layernorm_bwd   pair and dz read once, d pair written once.
The bytes are a floor, not a model: rf_pair_softmax_bwd reads d att twice, the second time from cache.
rf_sym_layernorm_bwd replaces a chain of existing launches, timed here too (and compared with it, relative L2):
  the symmetrising copy (rf_copy4d) + rf_axpby, rf_gemm for dz . w, rf_layernorm_bwd with unit gamma, the transposing copy +
  rf_axpby -- five passes over an fp32 [B, L, L, d_pair] tensor and three such intermediates.
One process; every variant is warmed; the variants take turns inside each repeat; device events around --launches calls of one
variant; median and spread (min, max) of the per-call time over --reps repeats.  Prints one JSON object; --out also writes it to a
file (profiles/r15_msa_pair_backward.json), keeping a "kernel_errors" entry the test suite may have put there
(tests/test_pair_softmax_bwd_gpu.py, RF_MSA_PAIR_BACKWARD_ERRORS).
    python tools/msa_pair_backward_bench.py [--out FILE] [--B 4 --N 128 --L 256 --d_msa 384 --d_pair 288 --layers 4]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import ops  # noqa: E402

F32 = torch.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--L", type=int, default=256)
    ap.add_argument("--d_msa", type=int, default=384)
    ap.add_argument("--d_pair", type=int, default=288)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.launches >= 10 and a.reps >= 3
    R.set_compute_dtype(torch.bfloat16)
    dev = "cuda"
    B, N, L, D, Dp, H, nl = a.B, a.N, a.L, a.d_msa, a.d_pair, 4, a.layers
    NZ = nl * H
    nzp = (NZ + 7) // 8 * 8
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    mod = R.MsaUpdateWithPair(D, Dp, H, n_encoder_layers=nl, p_dropout=0.0).to(dev).enable_backward()
    msa = torch.randn(B, N, L, D, generator=g).to(dev)
    pair = torch.randn(B, L, L, Dp, generator=g).to(dev)
    w = torch.randn(B, N, L, D, generator=g).to(dev)
    msa_g, pair_g = msa.clone().requires_grad_(), pair.clone().requires_grad_()
    # the kernels' operands
    logits = (torch.randn(B, L, L, NZ, generator=g) * 3).to(dev)
    datt = torch.randn(NZ, B, L, L, generator=g).to(dev)
    dz = torch.randn(B, L, L, NZ, generator=g).to(dev)
    wf = (torch.randn(NZ, Dp, generator=g) * Dp ** -0.5).to(dev)
    wf_t = wf.t().contiguous()
    one = ops.fill(torch.empty(Dp, device=dev, dtype=F32), 1.0)
    eps = 1e-5

    def forward():
        with torch.no_grad():
            mod(msa, pair)

    def forward_backward():
        for t in [msa_g, pair_g] + list(mod.parameters()):
            t.grad = None
        (mod(msa_g, pair_g) * w).sum().backward()

    def transposed(x):
        """x[b, j, i, :] as a new tensor (rf_copy4d)"""
        return ops.copy(x.transpose(1, 2), torch.empty_like(x))

    def chain():
        """rf_sym_layernorm_bwd's arithmetic on the launches the library already had"""
        sym = ops.axpby(pair, 0.5, transposed(pair), 0.5, torch.empty_like(pair))
        gz = ops.linear(dz, wf_t, None, out_dtype=F32, exact=True)   # [B,L,L,Dp] = dz . w
        ds, _, _ = ops.layernorm_bwd(sym, gz, one, eps=eps)
        return ops.axpby(ds, 0.5, transposed(ds), 0.5, torch.empty_like(ds))

    sm_bytes = 3 * logits.numel() * 4 + B * L * L * nzp * 2
    ln_bytes = 2 * pair.numel() * 4 + dz.numel() * 4
    copies = {}
    for name, nbytes in (("copy_of_pair_softmax_bwd_bytes", sm_bytes), ("copy_of_sym_layernorm_bwd_bytes", ln_bytes)):
        n = nbytes // 8   # fp32 elements: each is read once and written once
        copies[name] = (torch.randn(n, device=dev), torch.empty(n, device=dev))

    variants = {
        "forward": forward,
        "forward_backward": forward_backward,
        "pair_softmax_bwd": lambda: ops.pair_softmax_bwd(logits, datt, nz_pad=nzp),
        "copy_of_pair_softmax_bwd_bytes": lambda: ops.axpby(copies["copy_of_pair_softmax_bwd_bytes"][0], 1.0, None, 0.0,
                                                            copies["copy_of_pair_softmax_bwd_bytes"][1]),
        "sym_layernorm_bwd": lambda: ops.sym_layernorm_bwd(pair, dz, wf, eps=eps),
        "sym_layernorm_bwd_chain": chain,
        "copy_of_sym_layernorm_bwd_bytes": lambda: ops.axpby(copies["copy_of_sym_layernorm_bwd_bytes"][0], 1.0, None, 0.0,
                                                             copies["copy_of_sym_layernorm_bwd_bytes"][1]),
    }
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    fused, unfused = ops.sym_layernorm_bwd(pair, dz, wf, eps=eps).double(), chain().double()
    agreement = ((fused - unfused).norm() / unfused.norm()).item()
    del fused, unfused
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
    res = {"shape": {"B": B, "N": N, "L": L, "d_msa": D, "d_pair": Dp, "heads": H, "layers": nl},
           "dtype": "bfloat16", "device": torch.cuda.get_device_name(0), "launches_per_repeat": a.launches, "reps": a.reps,
           "unit": "us per call (device events around the calls of one repeat)",
           "peak_extra_bytes_forward_backward": peak, "msa_fp32_bytes": msa.numel() * 4, "pair_fp32_bytes": pair.numel() * 4}
    for name, ts in times.items():
        ts = sorted(ts)
        res[name] = {"median_us": ts[len(ts) // 2], "min_us": ts[0], "max_us": ts[-1]}
    res["backward_us_by_difference"] = res["forward_backward"]["median_us"] - res["forward"]["median_us"]
    for name, nbytes, what in (
            ("pair_softmax_bwd", sm_bytes, "logits and d att in, dz out in fp32, dz out in the 16-bit type (padded columns included)"),
            ("sym_layernorm_bwd", ln_bytes, "pair and dz in, d pair out")):
        copy = res[f"copy_of_{name}_bytes"]["median_us"]
        res[name].update(bytes_moved=nbytes, what=what, rate_TBps=nbytes / res[name]["median_us"] / 1e6,
                         times_the_copy=res[name]["median_us"] / copy)
        res[f"copy_of_{name}_bytes"].update(bytes_moved=nbytes, rate_TBps=nbytes / copy / 1e6)
    res["sym_layernorm_bwd_chain"].update(
        what="rf_copy4d + rf_axpby (symmetrise), rf_gemm (dz . w), rf_layernorm_bwd (unit gamma), rf_copy4d + rf_axpby",
        times_the_fused_kernel=res["sym_layernorm_bwd_chain"]["median_us"] / res["sym_layernorm_bwd"]["median_us"],
        rel_l2_fused_vs_chain=agreement)
    res["fused_is_faster_than_chain"] = res["sym_layernorm_bwd"]["median_us"] < res["sym_layernorm_bwd_chain"]["median_us"]
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
