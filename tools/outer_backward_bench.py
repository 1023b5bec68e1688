"""OuterProductMean forward / backward at the benchmark's pair shape, and the LayerNorm step of one backward slab both ways:
rf_layernorm_bwd_fused (one launch, in place) against the chain of the older engines (rf_layernorm, two casts to fp32,
rf_layernorm_bwd, a cast back).  Prints one JSON object; --out also writes it to a file (profiles/*outer_backward.json).
    python tools/outer_backward_bench.py [--out FILE] [--B 4 --N 128 --L 256]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import ops  # noqa: E402
from rosettafold_pytorch_amd.model import ln  # noqa: E402
from rosettafold_pytorch_amd.runtime import RT  # noqa: E402


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1], "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--L", type=int, default=256)
    ap.add_argument("--P", type=int, default=32)
    ap.add_argument("--dout", type=int, default=288)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    R.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    dev = "cuda"
    mod = R.OuterProductMean(a.P, a.dout).to(dev).enable_backward()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(a.B, a.N, a.L, a.P, generator=g).to(dev).requires_grad_()
    y = (0.1 * torch.randn(a.B, a.N, a.L, a.P, generator=g)).to(dev).requires_grad_()
    w = torch.randn(a.B, a.L, a.L, a.dout, generator=g).to(dev)
    res = {"shape": {"B": a.B, "N": a.N, "L": a.L, "P": a.P, "d_pair": a.dout}, "dtype": "bfloat16",
           "device": torch.cuda.get_device_name(0), "slab_rows": mod.backward_slab_rows(a.L, a.P),
           "slab_budget_bytes": RT.outer_bwd_slab_bytes}
    with torch.no_grad():
        res["forward"] = timed(lambda: mod(x, y), a.reps)

    def backward():
        out = mod(x, y)
        out.backward(w)

    for fused in (True, False):
        RT.outer_bwd_fused = fused
        out = mod(x, y)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out.backward(w)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before   # (on the first pass this holds x.grad and y.grad too)
        del out
        key = "backward_fused_ln" if fused else "backward_chain_ln"
        res[key] = timed(backward, a.reps, warmup=1)   # (forward + backward: the forward's median is reported above)
        res[key]["peak_extra_bytes"] = peak
    RT.outer_bwd_fused = True
    res["wide_tensor_fp32_bytes"] = a.B * a.L * a.L * a.P * a.P * 4

    # the LayerNorm step of one slab, both ways
    h, PP = res["slab_rows"], a.P * a.P
    lnm = mod.to_out[0]
    gamma, beta = lnm.weight.detach(), lnm.bias.detach()
    o = torch.randn(h, a.L, PP, generator=g).to(torch.bfloat16).to(dev)
    dz = torch.randn(h, a.L, PP, generator=g).to(torch.bfloat16).to(dev)

    def chain():
        z = ln(lnm, o)
        do32, _, _ = ops.layernorm_bwd(ops.cast(o, torch.float32), ops.cast(dz, torch.float32), gamma, eps=lnm.eps)
        return z, ops.cast(do32, torch.bfloat16)

    o2, dz2 = o.clone(), dz.clone()   # (in place: the timing does not depend on the values)
    res["slab_ln_step"] = {"rows": h * a.L, "D": PP,
                           "fused": timed(lambda: ops.layernorm_bwd_fused(o2, dz2, gamma, beta, eps=lnm.eps, dx=dz2, z=o2), 20, 5),
                           "fused_out_of_place": timed(lambda: ops.layernorm_bwd_fused(o, dz, gamma, beta, eps=lnm.eps), 20, 5),
                           "chain": timed(chain, 20, 5)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
