"""The fused tied MSA-row attention at chain lengths off 512 / 768 / 1024 and MSA depths off a multiple of 16 against the general
route on the same tree, and the whole-tile launches against another build of the library (the parent commit's, --parent-lib and
--parent-lib-f16) in the same process.  d_msa 384, 12 heads, B = 1, bf16 and fp16.  Every variant is timed in interleaved windows
(one window = --reps calls between two device events, after a warm-up of every shape; "graph_" variants replay the same call
captured into a graph, i.e. without the host's share of an eager call); per variant the minimum, the median and
the spread (max - min) / min of the windows' per-call times are reported.  Prints one JSON object; --out also writes it to a file
(profiles/*tied_long_ragged.json).
    python tools/tied_long_ragged_bench.py [--out FILE] [--parent-lib OLD/librfmi.so --parent-lib-f16 OLD/librfmi_f16.so]
Variants per dtype:
  A, N = 64, per L in --L:  "attend_fused" / "attend_general" = SoftTiedAttentionOverResidues.attend on the long-row route / on the
     general route (RT.tied_long_ragged off; at 512 / 768 / 1024, which that switch does not move, RT.fused_tied off), "logits" =
     the logits launch alone (ops.tied_logits_long, ops.tied_logits at whole tiles) on prebuilt head-major q | k;
     at 512 / 768 / 1024 also "logits_raw" / "parent_logits_raw" = rf_tied_logits through this build / the other one.
  B, L in {256, 137}, N in {100, 128}:  "attend_fused" / "attend_general" (RT.fused_tied off), "poswise" =
     ops.poswise_collapsed alone; at N = 128 also "poswise_raw" / "parent_poswise_raw"."""
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

D, H, DH = 384, 12, 32
WHOLE = (512, 768, 1024)


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


def graphed(fn):
    """fn captured into a graph (after one call on the capture stream: weight copies are prepared outside); returns the replay"""
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            keep = fn()
    torch.cuda.current_stream().wait_stream(side)
    return lambda graph=graph, keep=keep: graph.replay()


def other_build(path, names):
    old = C.CDLL(os.path.abspath(path))
    for n in names:
        getattr(old, n).argtypes = _lib.PROTOTYPES[n]
        getattr(old, n).restype = C.c_int
    return old


def variants_of(dt, a, parent):
    """name -> callable, for the compute dtype dt (already selected)"""
    dev = "cuda"
    torch.manual_seed(0)
    mod = R.SoftTiedAttentionOverResidues(D, H, 0.0, return_att=True).to(dev).eval()
    g = torch.Generator().manual_seed(0)
    v = {}

    def attend(xn, x_res, fused, general_by_fused_tied):
        def run():
            RT.tied_long_ragged = fused
            RT.fused_tied = fused or not general_by_fused_tied
            with torch.no_grad():
                return mod.attend(xn, x_res, True)
        return run

    def inputs(N, L_):
        x = torch.randn(1, N, L_, D, generator=g).to(dev)
        return ops.cast(x, dt), torch.zeros(1, N, L_, D, device=dev)

    N = 64
    for L_ in a.L:   # ---- A
        xn, x_res = inputs(N, L_)
        key = f"A_N{N}_L{L_}"
        v[key + "/attend_fused"] = attend(xn, x_res, True, L_ in WHOLE)
        v[key + "/attend_general"] = attend(xn, x_res, False, L_ in WHOLE)
        v[key + "/graph_attend_fused"] = graphed(v[key + "/attend_fused"])
        v[key + "/graph_attend_general"] = graphed(v[key + "/attend_general"])
        qk = (0.3 * torch.randn(1, N, 2 * H, L_, DH, generator=g)).to(dt).to(dev)
        att = torch.empty(1, H, L_, ops.tied_ld(L_), device=dev, dtype=dt)
        sym = torch.empty(1, L_, L_, H, device=dev)
        fn = ops.tied_logits if L_ in WHOLE else ops.tied_logits_long
        v[key + "/logits"] = (lambda fn=fn, qk=qk, att=att, sym=sym: fn(qk[:, :, :H], qk[:, :, H:], att, sym))
        if L_ in WHOLE:
            ws = torch.empty(H * L_ * L_, device=dev)
            st = _lib.I64x4(*qk[:, :, :H].stride()[:4])

            def raw(lib, qk=qk, att=att, sym=sym, ws=ws, st=st, N=N, L_=L_):
                rc = lib.rf_tied_logits(ops.ptr(qk[:, :, :H]), ops.ptr(qk[:, :, H:]), C.byref(st), None, None, 1.0, ops.ptr(att), ops.ptr(sym),
                                        H, 1, H, N, L_, DH, ops.ptr(ws), ws.numel(), ops.stream())
                assert rc == 0, rc
            v[key + "/logits_raw"] = (lambda f=raw: f(_lib.LIBS[ops.dcode(dt)]))
            if parent is not None:
                v[key + "/parent_logits_raw"] = (lambda f=raw: f(parent))
    for N in (100, 128):   # ---- B
        for L_ in (256, 137):
            xn, x_res = inputs(N, L_)
            key = f"B_N{N}_L{L_}"
            v[key + "/attend_fused"] = attend(xn, x_res, True, True)
            v[key + "/attend_general"] = attend(xn, x_res, False, True)
            v[key + "/graph_attend_fused"] = graphed(v[key + "/attend_fused"])
            v[key + "/graph_attend_general"] = graphed(v[key + "/attend_general"])
            u = (0.3 * torch.randn(1, L_, H, D, generator=g)).to(dt).to(dev)
            v[key + "/poswise"] = (lambda xn=xn, u=u: ops.poswise_collapsed(xn, u, DH ** -0.5))
            if N == 128:
                w = torch.empty(1, H, N, L_, device=dev)

                def raw(lib, xn=xn, u=u, w=w, N=N, L_=L_):
                    rc = lib.rf_poswise_collapsed(ops.ptr(xn), ops.ptr(u), ops.ptr(w), 1, N, L_, D, H, DH ** -0.5, ops.stream())
                    assert rc == 0, rc
                v[key + "/poswise_raw"] = (lambda f=raw: f(_lib.LIBS[ops.dcode(dt)]))
                if parent is not None:
                    v[key + "/parent_poswise_raw"] = (lambda f=raw: f(parent))
    return v


def checks_of(t, Ls):
    noise = max(x["spread"] for k, x in t.items() if k.endswith("_raw"))
    c = {"raw_window_spread_max": noise}
    for k in t:   # (a) the fused route against the general route of the same process: eager calls and graph replays
        if k.endswith("/attend_fused"):
            key = k.split("/")[0]
            f, gen = t[k]["min_ms"], t[key + "/attend_general"]["min_ms"]
            gf, gg = t[key + "/graph_attend_fused"]["min_ms"], t[key + "/graph_attend_general"]["min_ms"]
            c["a_" + key] = {"fused_min_ms": f, "general_min_ms": gen, "general_over_fused": gen / f,
                             "graph_fused_min_ms": gf, "graph_general_min_ms": gg, "graph_general_over_fused": gg / gf,
                             "fused_no_slower": f <= gen and gf <= gg}
    for r, w in ((511, 512), (1023, 1024)):   # (b) one residue short of a whole tile against the whole tile
        for what in ("attend_fused", "graph_attend_fused", "logits"):
            if r in Ls and w in Ls:
                x, y = t[f"A_N64_L{r}/{what}"]["min_ms"], t[f"A_N64_L{w}/{what}"]["min_ms"]
                c[f"b_{what}_L{r}_over_L{w}"] = {"ragged_min_ms": x, "whole_min_ms": y, "ratio": x / y}
    for k in t:   # (c) whole tiles and N = 128: this build against the other one, within the run's own repeat spread
        if "/parent_" in k:
            new = t[k.replace("parent_", "")]
            both = max(new["spread"], t[k]["spread"])
            c["c_" + k.split("/")[0] + "_" + k.split("/")[1].replace("parent_", "")] = {
                "new_min_ms": new["min_ms"], "parent_min_ms": t[k]["min_ms"], "ratio": new["min_ms"] / t[k]["min_ms"],
                "spread_of_the_two": both, "within_spread": abs(new["min_ms"] / t[k]["min_ms"] - 1) <= both}
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, nargs="+", default=[257, 300, 384, 437, 511, 512, 700, 768, 1000, 1023, 1024])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--parent-lib", default=None, help="another build of librfmi.so (bf16)")
    ap.add_argument("--parent-lib-f16", default=None, help="another build of librfmi_f16.so")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"shape": {"B": 1, "d_msa": D, "heads": H}, "device": torch.cuda.get_device_name(0), "reps_per_window": a.reps}
    names = ("rf_tied_logits", "rf_poswise_collapsed")
    for dt, tag, path in ((torch.bfloat16, "bfloat16", a.parent_lib), (torch.float16, "float16", a.parent_lib_f16)):
        R.set_compute_dtype(dt)
        variants = variants_of(dt, a, other_build(path, names) if path else None)
        for fn in variants.values():   # warm-up: every shape, every route
            fn()
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(a.windows):
            for k, fn in variants.items():
                times[k].append(window(fn, a.reps))
        RT.tied_long_ragged = RT.fused_tied = True
        t = {k: summary(x) for k, x in times.items()}
        res[tag] = {"times": t, "checks": checks_of(t, a.L)}
    R.set_compute_dtype(torch.bfloat16)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
