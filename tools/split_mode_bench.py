"""Cost of the "high" float32 matmul precision (split-bf16 GEMMs, RF_F32X3) on the GPU box.

    python tools/split_mode_bench.py [--config 2] [--steps 3]      # graphed forwards: bf16 | fp32 "highest" | fp32 "high"
    python tools/split_mode_bench.py --gemm                          # + rf_gemm alone at the fp32 mode's main shapes
    rocprofv3 --kernel-trace --stats -- python tools/split_mode_bench.py --modes fp32_high --steps 1   # where "high" spends its time

One process, one device: the three modes of the same model on the same inputs, each timed over --steps replays of one
hipGraph after a warm-up (what bench.py times for the bf16 headline).  Prints one JSON object; DESIGN.md quotes it."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import ops  # noqa: E402
from rosettafold_pytorch_amd import _lib as L  # noqa: E402

MODES = [("bf16", torch.bfloat16, "highest"), ("fp32_highest", torch.float32, "highest"), ("fp32_high", torch.float32, "high")]


def time_forward(model, inputs, dtype, precision, steps):
    R.set_compute_dtype(dtype)
    R.set_float32_matmul_precision(precision)
    try:
        with torch.no_grad():
            model(*inputs)  # warm-up: weight copies of this mode
            torch.cuda.synchronize()
            g = R.GraphedForward(model, *inputs)
            g(*inputs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                out = g(*inputs)
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0) / steps
            return ms, out[0]["dist"].float().clone()
    finally:
        R.set_float32_matmul_precision("highest")
        R.set_compute_dtype(torch.bfloat16)


def time_gemm(M, N, K, exact, reps=20):
    A = torch.randn(M, K, device="cuda")
    B = torch.randn(N, K, device="cuda")
    C = torch.empty(M, N, device="cuda")
    bias = torch.randn(N, device="cuda")
    R.set_compute_dtype(torch.float32)
    R.set_float32_matmul_precision("high")
    try:
        ops.gemm(A, B, C, M, N, K, bias=bias, exact=exact)
        fam = L.lib.rf_gemm_last_family()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            ops.gemm(A, B, C, M, N, K, bias=bias, exact=exact)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps, fam
    finally:
        R.set_float32_matmul_precision("highest")
        R.set_compute_dtype(torch.bfloat16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--gemm", action="store_true")
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--modes", default=",".join(m[0] for m in MODES), help="subset of bf16,fp32_highest,fp32_high (e.g. for a profiler run)")
    a = ap.parse_args()
    res = {"tool": "split_mode_bench", "config": a.config, "steps": a.steps}
    if not a.no_forward:
        c = bench.CONFIGS[a.config]
        cfg = dict(c["model"], d_input=21, p_dropout=0.0)
        torch.manual_seed(0)
        model = R.RoseTTAFold(**cfg).to("cuda").eval()
        inputs = bench.make_inputs(c["B"], c["N"], c["L"], 0, "cuda")
        res["B"], res["N"], res["L"] = c["B"], c["N"], c["L"]
        dist = {}
        for name, dt, prec in [m for m in MODES if m[0] in a.modes.split(",")]:
            ms, dist[name] = time_forward(model, inputs, dt, prec, a.steps)
            res[f"ms_{name}"] = round(ms, 1)
            print(f"{name}: {ms:.1f} ms per forward", file=sys.stderr, flush=True)
        if "fp32_highest" in dist and "fp32_high" in dist:
            res["high_over_highest"] = round(res["ms_fp32_high"] / res["ms_fp32_highest"], 3)
        ref = dist.get("fp32_highest")
        for name in [n for n in ("bf16", "fp32_high") if n in dist and ref is not None]:
            d, ref = dist[name].double(), ref.double()
            res[f"dist_rel_l2_{name}_vs_highest"] = ((d - ref).norm() / ref.norm()).item()
            res[f"dist_argmax_{name}_vs_highest"] = (d.argmax(-1) == ref.argmax(-1)).float().mean().item()
    if a.gemm:
        # fp32-mode shapes at config 2 (B=4, N=128, L=256): pair-track projections (rows B L L) and MSA-track ones (rows B N L)
        shapes = [(262144, 288, 288), (262144, 72, 288), (131072, 384, 384), (131072, 1536, 384), (131072, 384, 1536),
                  (65536, 288, 2592)]
        rows = []
        for M, N, K in shapes:
            te, fe = time_gemm(M, N, K, True)
            ts, fs = time_gemm(M, N, K, False)
            rows.append({"M": M, "N": N, "K": K, "ms_exact": round(te, 3), "ms_split": round(ts, 3), "ratio": round(ts / te, 3),
                         "families": [fe, fs], "tflops_split": round(2 * M * N * K / ts / 1e9, 1)})
            print(rows[-1], file=sys.stderr, flush=True)
        res["gemm"] = rows
    print(json.dumps(res))


if __name__ == "__main__":
    main()
