"""The fused outer product at ragged chain lengths and MSA depths against the general (two-GEMM) route on the same tree, and the
whole-tile call against another build of the library (the parent commit's, --parent-lib) in the same process.  Every variant is
timed in interleaved windows (one window = --reps calls between two device events, after a warm-up of every shape); per variant
the minimum, the median and the spread (max - min) / min of the windows' per-call times are reported.  Prints one JSON object;
--out also writes it to a file (profiles/*outer_ragged.json).
    python tools/outer_ragged_bench.py [--out FILE] [--parent-lib OLD/librfmi.so] [--B 4 --reps 100 --windows 7]
Variants per (N, L): "module_fused" / "module_general" = OuterProductMean.forward (operand transposes + the route; RT.fused_outer
on / off), "kernel" = ops.outer_fused alone on prebuilt operands; at N = 128, L = 256 also "kernel_sq" / "parent_kernel_sq" =
rf_outer_product_ln_linear through this build / the other one."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import _lib, ops  # noqa: E402
from rosettafold_pytorch_amd.runtime import RT  # noqa: E402

P, DOUT = 32, 288


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def summary(ts):
    s = sorted(ts)
    return {"min_ms": s[0], "median_ms": s[len(s) // 2], "max_ms": s[-1], "spread": (s[-1] - s[0]) / s[0], "windows": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--N", type=int, nargs="+", default=[128, 100])
    ap.add_argument("--L", type=int, nargs="+", default=[256, 255, 250, 137])
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--parent-lib", default=None, help="another build of librfmi.so (bf16) to time rf_outer_product_ln_linear of")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    R.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    dev = "cuda"
    mod = R.OuterProductMean(P, DOUT).to(dev)
    wp, s_, c_ = mod._fold()
    eps = mod.to_out[0].eps
    g = torch.Generator().manual_seed(0)
    variants = {}   # name -> callable

    def module(x, y, fused):
        def run():
            RT.fused_outer = fused
            with torch.no_grad():
                return mod(x, y)
        return run

    for N in a.N:
        for L_ in a.L:
            x = torch.randn(a.B, N, L_, P, generator=g).to(dev)
            y = (0.1 * torch.randn(a.B, N, L_, P, generator=g)).to(dev)
            xt, yt, _ = ops.outer_operands(x, y, torch.bfloat16, ops.outer_depth(N))
            out = torch.empty(a.B, L_, L_, DOUT, device=dev, dtype=torch.float32)
            key = f"N{N}_L{L_}"
            variants[key + "/module_fused"] = module(x, y, True)
            variants[key + "/module_general"] = module(x, y, False)
            variants[key + "/kernel"] = (lambda xt=xt, yt=yt, out=out: ops.outer_fused(xt, yt, wp, s_, c_, out, eps))
            if N == 128 and L_ % 16 == 0:
                def square(lib, xt=xt, yt=yt, out=out, L_=L_, N=N):
                    rc = lib.rf_outer_product_ln_linear(ops.ptr(xt), ops.ptr(yt), ops.ptr(wp), ops.ptr(s_), ops.ptr(c_), ops.ptr(out),
                                                        a.B, L_, N, P, DOUT, eps, None, None, 0.0, None, 0, ops.stream())
                    assert rc == 0, rc
                variants[key + "/kernel_sq"] = (lambda f=square: f(_lib.LIBS[_lib.RF_BF16]))
                if a.parent_lib:
                    old = C.CDLL(os.path.abspath(a.parent_lib))
                    old.rf_outer_product_ln_linear.argtypes = _lib.PROTOTYPES["rf_outer_product_ln_linear"]
                    old.rf_outer_product_ln_linear.restype = C.c_int
                    variants[key + "/parent_kernel_sq"] = (lambda f=square, old=old: f(old))
    for fn in variants.values():   # warm-up: every shape, every route
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.windows):
        for k, fn in variants.items():
            times[k].append(window(fn, a.reps))
    RT.fused_outer = True
    res = {"shape": {"B": a.B, "P": P, "d_pair": DOUT}, "dtype": "bfloat16", "device": torch.cuda.get_device_name(0),
           "reps_per_window": a.reps, "times": {k: summary(v) for k, v in times.items()}}
    t = res["times"]
    noise = max(v["spread"] for k, v in t.items() if k.endswith(("/kernel", "kernel_sq")))
    res["kernel_window_spread_max"] = noise
    checks = {}
    if "N128_L256/parent_kernel_sq" in t:   # (a) whole tiles: this build against the other one
        new, old = t["N128_L256/kernel_sq"]["min_ms"], t["N128_L256/parent_kernel_sq"]["min_ms"]
        checks["a_full_tile_vs_parent"] = {"new_min_ms": new, "parent_min_ms": old, "ratio": new / old, "within_noise": new <= old * (1 + noise)}
    for N in a.N:   # (b) the same tile count: L = 255 against L = 256
        if f"N{N}_L255/kernel" in t and f"N{N}_L256/kernel" in t:
            r, f = t[f"N{N}_L255/kernel"]["min_ms"], t[f"N{N}_L256/kernel"]["min_ms"]
            checks[f"b_N{N}_L255_vs_L256"] = {"L255_min_ms": r, "L256_min_ms": f, "ratio": r / f, "within_noise": r <= f * (1 + noise)}
    for k in t:     # (c) fused against general, whole module call
        if k.endswith("/module_fused"):
            key = k.split("/")[0]
            f, gen = t[k]["min_ms"], t[key + "/module_general"]["min_ms"]
            checks["c_" + key] = {"fused_min_ms": f, "general_min_ms": gen, "general_over_fused": gen / f, "fused_wins": f < gen}
    res["checks"] = checks
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
