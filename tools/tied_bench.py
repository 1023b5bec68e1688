#!/usr/bin/env python3
"""Tied MSA-row attention core at the bench shape (run on the GPU box): round-2 head-major kernels vs the round-1 path."""
import os, sys, math, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rosettafold_pytorch_amd as R
from rosettafold_pytorch_amd import ops
def timeit(fn, iters=20):
    fn(); torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / iters
if "--ragged" in sys.argv:
    # python tools/tied_bench.py --ragged [out.json]: SoftTiedAttentionOverResidues.attend (projections, position weights and output
    # projection included) at the config-2 MSA shape, bf16, at chain lengths that fill no tile of the fused kernels (and at 256 and
    # 304 for scale): the route the model takes against the general path (rf_gemm logits + rf_tied_softmax + v^T GEMM + generic
    # A.V; RT.tied_v2 = False), and the same with the symmetrised map.  Eager launches, min of 3 windows.
    import json
    B, H, N, D = 4, 12, 128, 384
    m = R.SoftTiedAttentionOverResidues(D, H, 0.0, return_att=True).cuda()
    def attend_ms(L, v2, want_att, iters):
        xn = torch.randn(B, N, L, D, device="cuda").bfloat16()
        res = torch.zeros(B, N, L, D, device="cuda")
        R.RT.tied_v2 = v2
        try:
            return min(timeit(lambda: m.attend(xn, res, want_att), iters) for _ in range(3))
        except ops.L.RfmiError as e:  # (a tree without the padded leading dimension refuses L % 8 != 0: RF_EALIGN)
            print(f"   tied_v2={v2} refused: {e}", flush=True)
            return None
        finally:
            R.RT.tied_v2 = True
    rows = []
    for L in (100, 137, 200, 255, 256, 304, 700, 17, 40, 72):  # (the last three: where a floor R.model.TIED_RAGGED_MIN_L would sit)
        fused_route = L in ops.TIED_TILES or (L >= R.model.TIED_RAGGED_MIN_L and
                                              ops.tied_fused_applies(L, N, torch.bfloat16, w=not m.folds_weights(B * N * L)))
        iters = 5 if L >= 300 else 20
        for want_att in (False, True):
            td, tg = attend_ms(L, True, want_att, iters), attend_ms(L, False, want_att, iters)
            rows.append(dict(L=L, B=B, N=N, D=D, H=H, want_att=want_att, default_route="fused" if fused_route else "general",
                             default_ms=td, general_ms=tg, general_over_default=tg / td if td and tg else None))
            f = lambda t: f"{t*1e3:.0f} us" if t else "refused"  # noqa: E731
            print(f"L={L} att_sym={want_att}: default ({rows[-1]['default_route']}) {f(td)}, general {f(tg)}", flush=True)
    out = [a_ for a_ in sys.argv[1:] if a_.endswith(".json")]
    if out:
        json.dump(rows, open(out[0], "w"), indent=1)
    sys.exit(0)
B, H, N, L, dh = 4, 12, 128, 256, 32
D = H * dh
fl = 2.0 * B * H * L * L * N * dh
qkv = (torch.randn(B, N, 3 * H, L, dh, device="cuda") * (0.9 / math.sqrt(math.sqrt(N)))).bfloat16()
q, k, v = qkv[:, :, :H], qkv[:, :, H:2 * H], qkv[:, :, 2 * H:]
w = torch.rand(B, H, N, L, device="cuda").softmax(2).contiguous()
att = torch.empty(B, H, L, L, device="cuda", dtype=torch.bfloat16)
sym = torch.empty(B, L, L, H, device="cuda", dtype=torch.float32)
out = torch.empty(B, N, L, D, device="cuda", dtype=torch.bfloat16)
o5 = out.view(B, N, L, H, dh).permute(0, 1, 3, 2, 4)
import ctypes as C
from rosettafold_pytorch_amd._lib import lib, I64x4, I64x3
t_all = timeit(lambda: ops.tied_attention(q, k, v, o5, att, w=w, qscale=0.17))
print(f"v2 core (logits+softmax with weights, A.V): {t_all*1e3:.1f} us = {2*fl/t_all/1e9:.0f} TF/s (51.5 GF)")
vs, os_ = I64x4(*v.stride()[:4]), I64x4(*o5.stride()[:4])
t_av = timeit(lambda: lib.rf_tied_av(ops.ptr(att), ops.ptr(v), C.byref(vs), ops.ptr(out), C.byref(os_), B, H, N, L, dh, ops.stream()))
print(f"   A.V kernel alone: {t_av*1e3:.1f} us = {fl/t_av/1e9:.0f} TF/s; logits+softmax: {(t_all-t_av)*1e3:.1f} us = {fl/(t_all-t_av)/1e9:.0f} TF/s")
t_one = timeit(lambda: ops.tied_attention(q, k, v, o5, att, w=w, qscale=0.17, partial_ws=False))
print(f"   one-pass logits kernel instead of the contraction-split one: {t_one*1e3:.1f} us -> logits+softmax {(t_one-t_av)*1e3:.1f} us")
t_nw = timeit(lambda: ops.tied_attention(q, k, v, o5, att, w=None))
print(f"   without position weights (q pre-scaled): {t_nw*1e3:.1f} us -> logits+softmax {(t_nw-t_av)*1e3:.1f} us")
t_sym = timeit(lambda: ops.tied_attention(q, k, v, o5, att, w=w, qscale=0.17, att_sym=sym))
print(f"   with the symmetrised map: {t_sym*1e3:.1f} us")
xn = torch.randn(B, N, L, D, device="cuda").bfloat16()
u = (torch.randn(B, L, H, D, device="cuda") * 0.1).bfloat16()
print(f"position weights (collapsed, MFMA): {timeit(lambda: ops.poswise_collapsed(xn, u, 0.17))*1e3:.1f} us")
wq = (torch.randn(3 * D, D, device="cuda") * 0.05).bfloat16()
bq = torch.randn(3 * D, device="cuda")
hm = torch.empty(B, N, 3 * H, L, dh, device="cuda", dtype=torch.bfloat16)
t_p = timeit(lambda: ops.gemm(xn, wq, hm, B * N * L, 3 * D, D, bias=bq, c_row=(L, 3 * H * L * dh, dh), c_col=(dh, L * dh)))
plain = torch.empty(B, N, L, 3 * D, device="cuda", dtype=torch.bfloat16)
t_pp = timeit(lambda: ops.linear(xn, wq, bq, out=plain))
print(f"q|k|v projection head-major: {t_p*1e3:.1f} us; plain layout: {t_pp*1e3:.1f} us")
# round-1 path for comparison
qkp = (torch.randn(B, N, L, 3 * D, device="cuda") * (0.6 / math.sqrt(N))).bfloat16()
t1 = timeit(lambda: ops.tied_logits_softmax(qkp, qkp[..., D:], N * L * 3 * D, L * 3 * D, 3 * D, att, None, B, H, N, L, dh))
print(f"round-1 logits+softmax on [B,N,L,3D]: {t1*1e3:.1f} us = {fl/t1/1e9:.0f} TF/s")
# whole layer through the model classes
m = R.EncoderLayer(d_msa=D, d_ff=4 * D, n_heads=H, p_dropout=0.0, tied=True, return_att=True).cuda()
x = torch.randn(B, N, L, D, device="cuda")
for v2 in (True, False):
    R.RT.tied_v2 = v2
    print(f"tied encoder layer, tied_v2={v2}: {timeit(lambda: m.run(x, want_att=False), 10)*1e3:.1f} us")
R.RT.tied_v2 = True
