"""MsaEmbedding and PairEmbedding with their backward pass (enable_backward) at the benchmark config's shape (config 2: B=4,
N=128, L=256, d_msa=384, d_pair=288, bf16): per module the forward (no_grad), forward + backward through autograd and the
backward's peak extra memory, and the two kernels the backward adds, each next to the bytes it must move and to a bare rf_axpby
copy that moves as many bytes (read + written) in the same run:
  rf_embedding_bwd     the [B, N, L, d_msa] gradient read once; d table and d query_enc written (and the fp64 partials of the
                       blocks written and read back, which the byte count leaves out: it is a floor);
                       timed without and with a dropout mask to replay (p = 0.1);
  rf_pair_axis_sums    the [B, L, L, d_pair] gradient read once; rows, cols, dsep and dbias written (partials left out likewise).
One process; every variant is warmed; the variants take turns inside each repeat; device events around --launches calls of one
variant; median and spread (min, max) of the per-call time over --reps repeats.  Prints one JSON object; --out also writes it to a
file (profiles/r20_embedding_backward.json), keeping a "kernel_errors" entry the test suite may have put there
(tests/test_embedding_bwd_gpu.py, RF_EMBEDDING_BACKWARD_ERRORS).
    python tools/embedding_backward_bench.py [--out FILE] [--B 4 --N 128 --L 256 --d_msa 384 --d_pair 288]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import _lib, ops  # noqa: E402

F32 = torch.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--L", type=int, default=256)
    ap.add_argument("--d_msa", type=int, default=384)
    ap.add_argument("--d_pair", type=int, default=288)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.launches >= 10 and a.reps >= 3
    R.set_compute_dtype(torch.bfloat16)
    dev = "cuda"
    B, N, L, D, Dp, V = a.B, a.N, a.L, a.d_msa, a.d_pair, 21
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    msa_mod = R.MsaEmbedding(d_input=V, d_msa=D, max_len=L + 4).to(dev).enable_backward()
    pair_mod = R.PairEmbedding(d_input=V, d_pair=Dp, max_len=L + 4).to(dev).enable_backward()
    msa = torch.randint(0, V, (B, N, L), generator=g).to(dev)
    seq = msa[:, 0].contiguous()
    aa_idx = torch.arange(L).unsqueeze(0).repeat(B, 1).to(dev)
    w_msa = torch.randn(B, N, L, D, generator=g).to(dev)
    w_pair = torch.randn(B, L, L, Dp, generator=g).to(dev)
    drop = (0.1, 1234, 77)

    def forward(mod, *inputs):
        with torch.no_grad():
            mod(*inputs)

    def forward_backward(mod, w, *inputs):
        for t in mod.parameters():
            t.grad = None
        (mod(*inputs) * w).sum().backward()

    emb_bytes = w_msa.numel() * 4 + msa.numel() * 8 + (V + 2) * D * 4
    pas_bytes = w_pair.numel() * 4 + 2 * B * L * Dp * 4 + 2 * Dp * 4
    copies = {}
    for name, nbytes in (("copy_of_embedding_bwd_bytes", emb_bytes), ("copy_of_pair_axis_sums_bytes", pas_bytes)):
        n = nbytes // 8   # fp32 elements: each is read once and written once
        copies[name] = (torch.randn(n, device=dev), torch.empty(n, device=dev))

    variants = {
        "msa_forward": lambda: forward(msa_mod, msa, aa_idx),
        "msa_forward_backward": lambda: forward_backward(msa_mod, w_msa, msa, aa_idx),
        "pair_forward": lambda: forward(pair_mod, seq, aa_idx),
        "pair_forward_backward": lambda: forward_backward(pair_mod, w_pair, seq, aa_idx),
        "embedding_bwd": lambda: ops.embedding_bwd(msa, w_msa, V, query=(N, L)),
        "embedding_bwd_dropout": lambda: ops.embedding_bwd(msa, w_msa, V, query=(N, L), drop=drop),
        "copy_of_embedding_bwd_bytes": lambda: ops.axpby(copies["copy_of_embedding_bwd_bytes"][0], 1.0, None, 0.0,
                                                         copies["copy_of_embedding_bwd_bytes"][1]),
        "pair_axis_sums": lambda: ops.pair_axis_sums(w_pair, aa_idx),
        "copy_of_pair_axis_sums_bytes": lambda: ops.axpby(copies["copy_of_pair_axis_sums_bytes"][0], 1.0, None, 0.0,
                                                          copies["copy_of_pair_axis_sums_bytes"][1]),
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
    peaks = {}
    for name in ("msa_forward_backward", "pair_forward_backward"):
        variants[name]()
        for mod in (msa_mod, pair_mod):
            for t in mod.parameters():
                t.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        variants[name]()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
    res = {"shape": {"B": B, "N": N, "L": L, "d_msa": D, "d_pair": Dp, "d_input": V},
           "dtype": "bfloat16", "device": torch.cuda.get_device_name(0), "launches_per_repeat": a.launches, "reps": a.reps,
           "unit": "us per call (device events around the calls of one repeat)",
           "peak_extra_bytes_msa_forward_backward": peaks["msa_forward_backward"],
           "peak_extra_bytes_pair_forward_backward": peaks["pair_forward_backward"],
           "msa_gradient_fp32_bytes": w_msa.numel() * 4, "pair_gradient_fp32_bytes": w_pair.numel() * 4,
           "embedding_bwd_workspace_bytes": int(_lib.lib.rf_embedding_bwd_ws_bytes(B * N * L, D, V)),
           "pair_axis_sums_workspace_bytes": int(_lib.lib.rf_pair_axis_sums_ws_bytes(B, L, Dp))}
    for name, ts in times.items():
        ts = sorted(ts)
        res[name] = {"median_us": ts[len(ts) // 2], "min_us": ts[0], "max_us": ts[-1]}
    for mod in ("msa", "pair"):
        res[f"{mod}_backward_us_by_difference"] = res[f"{mod}_forward_backward"]["median_us"] - res[f"{mod}_forward"]["median_us"]
    for name, copy_name, nbytes, what in (
            ("embedding_bwd", "embedding_bwd", emb_bytes, "the gradient and the tokens in, d table and d query_enc out"),
            ("embedding_bwd_dropout", "embedding_bwd", emb_bytes, "the same with the mask of p = 0.1 replayed in the kernel"),
            ("pair_axis_sums", "pair_axis_sums", pas_bytes, "the gradient in, rows, cols, dsep and dbias out")):
        copy = res[f"copy_of_{copy_name}_bytes"]["median_us"]
        res[name].update(bytes_moved=nbytes, what=what, rate_TBps=nbytes / res[name]["median_us"] / 1e6,
                         times_the_copy=res[name]["median_us"] / copy)
        res[f"copy_of_{copy_name}_bytes"].update(bytes_moved=nbytes, rate_TBps=nbytes / copy / 1e6)
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
