"""GNormBias, G1x1SE3, GAttentiveSelfInt and GMABSE3 with their backward pass (enable_backward) at the structure track's shape of
the benchmark config (config 2: B=4, L=256, a kNN graph with k=128 on a random-walk chain, 16 / 16 channels, d_state=32): per
module the forward (no_grad) and forward + backward through autograd, and the five kernels the backward adds, each next to the
bytes it must move and to a bare rf_axpby copy that moves as many bytes (read + written) in the same run:
  rf_se3_attention_bwd    k, v, q, g and the eid map in; dk, dv, dq out (4 heads, 4 / 4 channels, the graph's edges);
  rf_se3_norm_bias_bwd    v, g in, dv out (degree 1, 16 channels; the fp64 terms of dbias left out: the count is a floor);
  rf_se3_gram_bwd         ds and v in, dv out (degree 0, 48 channels);
  rf_se3_attn_apply_bwd   att, x, g in; datt, dx out (degree 0, 48 -> 32);
  rf_layernorm_act_bwd    x and g in, dx out (rows = nodes, D = 48^2; x and g are read a second time for dgamma / dbeta, and the
                          partials are written: left out likewise).
The modules are the final layer's GAttentiveSelfInt ({0: 48, 1: 19} -> {0: 32, 1: 3}), a middle layer's G1x1SE3 projection
({0: 20, 1: 20} -> {0: 16, 1: 16}), GNormBias({0: 16, 1: 16}) and the 4-head GMABSE3 with its skip.  fp32 in every mode.
One process; every variant is warmed; the variants take turns inside each repeat; device events around --launches calls of one
variant; median and spread (min, max) of the per-call time over --reps repeats.  Prints one JSON object; --out also writes it to a
file (profiles/r22_se3_node_backward.json), keeping a "kernel_errors" entry the test suite may have put there
(tests/test_se3_bwd_kernels_gpu.py, RF_SE3_BACKWARD_ERRORS).
    python tools/se3_node_backward_bench.py [--out FILE] [--B 4 --L 256 --k 128]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import _lib, ops, structure as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--L", type=int, default=256)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.launches >= 10 and a.reps >= 3
    R.set_compute_dtype(torch.bfloat16)
    dev = "cuda"
    B, L, V = a.B, a.L, a.B * a.L
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    steps = torch.randn(B, L, 3, generator=g)
    ca = torch.cumsum(3.8 * steps / steps.norm(dim=-1, keepdim=True), 1)
    xyz = (ca[:, :, None, :] + 0.5 * torch.randn(B, L, 3, 3, generator=g)).to(dev).contiguous()
    aa_idx = torch.arange(L).unsqueeze(0).repeat(B, 1).to(dev)
    graph = S.build_graph(xyz, rn(B, L, L, 8), aa_idx, a.k)
    S.check_edge_capacity()
    n, cap = int(graph["count"][0]), graph["cap"]

    norm = S.GNormBias({0: 16, 1: 16}).to(dev).enable_backward()
    g1x1 = S.G1x1SE3({0: 20, 1: 20}, {0: 16, 1: 16}).to(dev).enable_backward()
    selfint = S.GAttentiveSelfInt({0: 48, 1: 19}, {0: 32, 1: 3}).to(dev).enable_backward()
    gmab = S.GMABSE3({0: 4, 1: 4}, {0: 4, 1: 4}, n_heads=4).to(dev).enable_backward()
    fiber = lambda f: {d: rn(V, m, 2 * d + 1).requires_grad_() for d, m in f.items()}  # noqa: E731
    edge = lambda f: {d: rn(cap, m, 2 * d + 1).requires_grad_() for d, m in f.items()}  # noqa: E731
    h_norm, h_1x1, h_si = fiber({0: 16, 1: 16}), fiber({0: 20, 1: 20}), fiber({0: 48, 1: 19})
    att_in = (edge({0: 4, 1: 4}), edge({0: 4, 1: 4}), fiber({0: 4, 1: 4}), graph, fiber({0: 16, 1: 16}))

    def forward(mod, *inputs):
        with torch.no_grad():
            mod(*inputs)

    def forward_backward(mod, *inputs):
        leaves = [t for x in inputs if x is not graph for t in x.values()]
        for t in list(mod.parameters()) + leaves:      # no accumulation into an earlier call's .grad
            t.grad = None
        sum(o.sum() for o in mod(*inputs).values()).backward()

    d = lambda t: t.detach()  # noqa: E731
    (v_e, k_e, q_n, _, _) = att_in
    g_att = {0: rn(V, 4, 1), 1: rn(V, 4, 3)}
    v1, g1 = d(h_norm[1]), rn(V, 16, 3)
    bias1 = norm.bias["1"].detach().reshape(-1)
    v0 = d(h_si[0])
    ds, att, g_out = rn(V, 48 * 48), rn(V, 32 * 48), rn(V, 32, 1)
    gamma, beta = torch.ones(48 * 48, device=dev), torch.zeros(48 * 48, device=dev)
    nbytes = {
        "se3_attention_bwd": 4 * (2 * n * (4 + 12) * 2 + V * (4 + 12) * 3 + B * L * L),
        "se3_norm_bias_bwd": 4 * 3 * V * 16 * 3,
        "se3_gram_bwd": 4 * (V * 48 * 48 + 2 * V * 48),
        "se3_attn_apply_bwd": 4 * (2 * V * 32 * 48 + 2 * V * 48 + V * 32),
        "layernorm_act_bwd": 4 * 3 * V * 48 * 48,
    }
    kernels = {
        "se3_attention_bwd": lambda: ops.se3_attention_bwd(d(k_e[0]), d(k_e[1]), d(q_n[0]), d(q_n[1]), d(v_e[0]), d(v_e[1]),
                                                           graph["eid"], g_att[0], g_att[1], 4, 4, 4, 4, 4, V, L),
        "se3_norm_bias_bwd": lambda: ops.se3_norm_bias_bwd(v1, bias1, g1, 1),
        "se3_gram_bwd": lambda: ops.se3_gram_bwd(v0, ds, 0),
        "se3_attn_apply_bwd": lambda: ops.se3_attn_apply_bwd(att, v0, g_out, 32, 0),
        "layernorm_act_bwd": lambda: ops.layernorm_act_bwd(ds, ds, gamma, beta, act=_lib.ACT_LEAKY),
    }
    copies = {name: (torch.randn(nb // 8, device=dev), torch.empty(nb // 8, device=dev)) for name, nb in nbytes.items()}
    variants = {
        "norm_bias_forward": lambda: forward(norm, h_norm), "norm_bias_forward_backward": lambda: forward_backward(norm, h_norm),
        "g1x1_forward": lambda: forward(g1x1, h_1x1), "g1x1_forward_backward": lambda: forward_backward(g1x1, h_1x1),
        "selfint_forward": lambda: forward(selfint, h_si), "selfint_forward_backward": lambda: forward_backward(selfint, h_si),
        "gmab_forward": lambda: forward(gmab, *att_in), "gmab_forward_backward": lambda: forward_backward(gmab, *att_in),
    }
    for name, fn in kernels.items():
        variants[name] = fn
        variants[f"copy_of_{name}_bytes"] = (lambda c: lambda: ops.axpby(c[0], 1.0, None, 0.0, c[1]))(copies[name])
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
    res = {"shape": {"B": B, "L": L, "k": a.k, "nodes": V, "edges": n, "edge_capacity": cap, "channels": [16, 16], "d_state": 32},
           "dtype": "float32 (the structure track, under every compute mode)", "device": torch.cuda.get_device_name(0),
           "launches_per_repeat": a.launches, "reps": a.reps, "unit": "us per call (device events around the calls of one repeat)",
           "norm_bias_bwd_workspace_bytes": int(_lib.lib.rf_se3_norm_bias_bwd_ws_bytes(V, 16, 1)),
           "layernorm_act_bwd_workspace_bytes": int(_lib.lib.rf_layernorm_act_bwd_ws_bytes(V, 48 * 48))}
    for name, ts in times.items():
        ts = sorted(ts)
        res[name] = {"median_us": ts[len(ts) // 2], "min_us": ts[0], "max_us": ts[-1]}
    for mod in ("norm_bias", "g1x1", "selfint", "gmab"):
        res[f"{mod}_backward_us_by_difference"] = res[f"{mod}_forward_backward"]["median_us"] - res[f"{mod}_forward"]["median_us"]
    for name, nb in nbytes.items():
        copy = res[f"copy_of_{name}_bytes"]["median_us"]
        res[name].update(bytes_moved=nb, rate_TBps=nb / res[name]["median_us"] / 1e6, times_the_copy=res[name]["median_us"] / copy)
        res[f"copy_of_{name}_bytes"].update(bytes_moved=nb, rate_TBps=nb / copy / 1e6)
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
