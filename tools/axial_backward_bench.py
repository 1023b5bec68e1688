"""Pair axial-attention backward at the config-2 pair shape (B = 4, L = 256, d_pair = 288, 8 heads, 4 layers; bf16 by default):
device-event times of the stack's forward with recording off, its forward with recording on (enable_backward + grad mode) and
the backward, all in one run after warm-up; plus the memory the recording forward leaves held for the backward (the tape).
Prints one JSON line.  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python ...`.

    python tools/axial_backward_bench.py [--B 4] [--L 256] [--C 288] [--heads 8] [--layers 4] [--dtype bf16|fp16|fp32]
                                         [--steps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rosettafold_pytorch_amd as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--L", type=int, default=256)
    ap.add_argument("--C", type=int, default=288)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("axial_backward_bench.py needs a GPU")
    R.set_compute_dtype({"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype])
    torch.manual_seed(0)
    mod = R.PairUpdateWithAxialAttention(a.C, 4 * a.C, a.heads, 0.1, a.layers).cuda()
    pair = torch.randn(a.B, a.L, a.L, a.C, device="cuda")
    gout = torch.randn(a.B, a.L, a.L, a.C, device="cuda")

    def fwd_plain():
        with torch.no_grad():
            return mod(pair)

    def fwd_rec():
        return mod(pair)

    def bwd(out):
        out.backward(gout)

    def timed(fn, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ts = []
        for _ in range(n):
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]))
        return ts

    mod.enable_backward()
    for _ in range(a.warmup):
        fwd_plain()
        bwd(fwd_rec())
    torch.cuda.synchronize()
    t_plain = timed(fwd_plain, a.steps)
    t_rec, t_bwd = [], []
    saved = 0
    for _ in range(a.steps):
        for p in mod.parameters():
            p.grad = None
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        holder = {}
        t_rec += timed(lambda: holder.update(out=fwd_rec()), 1)
        saved = max(saved, torch.cuda.memory_allocated() - m0 - holder["out"].numel() * 4)
        t_bwd += timed(lambda: bwd(holder.pop("out")), 1)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    print(json.dumps({"tool": "axial_backward_bench", "B": a.B, "L": a.L, "C": a.C, "heads": a.heads, "layers": a.layers,
                      "dtype": a.dtype, "steps": a.steps, "fwd_plain_ms": round(med(t_plain), 3),
                      "fwd_record_ms": round(med(t_rec), 3), "backward_ms": round(med(t_bwd), 3),
                      "backward_over_fwd": round(med(t_bwd) / med(t_plain), 3), "tape_bytes_GB": round(saved / 1e9, 3),
                      "peak_allocated_GB": round(torch.cuda.max_memory_allocated() / 1e9, 3)}))


if __name__ == "__main__":
    main()
