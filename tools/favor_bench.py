import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rosettafold_pytorch_amd as R
from rosettafold_pytorch_amd import ops
def timeit(fn, iters=10):
    fn(); torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / iters
torch.manual_seed(0)
if "--ragged" in sys.argv:
    # python tools/favor_bench.py --ragged [out.json]: PerformerSelfAttention.attend (q|k|v projection included) with the fused kernel
    # against the unfused chain, bf16, at lengths that are no multiple of the kernel's tiles; then the sweep the floor
    # ops.FAVOR_FUSED_MIN_LS is read from (pair layout, both axes, floor bypassed).  Eager launches, min of 3 windows.
    import json
    ops.FAVOR_FUSED_MIN_LS = 1
    def attend_ms(m, B, L1, L2, D, axis, fused, iters):
        xn = torch.randn(B, L1, L2, D, device="cuda").bfloat16()
        res = torch.zeros(B, L1, L2, D, device="cuda")
        R.RT.fused_favor = fused
        try:
            return min(timeit(lambda: m.attend(xn, res, axis), iters) for _ in range(3))
        except ops.L.RfmiError as e:  # the 16-bit unfused chain takes multiples of 8 only (RF_EALIGN): nothing to time
            print(f"   {'fused' if fused else 'unfused'} route refused: {e}", flush=True)
            return None
        finally:
            R.RT.fused_favor = True
    rows = []
    shapes = [(f"pair {ax} L={L}", True, 4, L, L, 288, 8, a_) for L in (200, 256, 300, 304, 700, 704) for ax, a_ in (("row", 1), ("col", 2))]
    shapes += [("msa col N=100 L=200", False, 4, 100, 200, 384, 12, 1), ("msa col N=104 L=200", False, 4, 104, 200, 384, 12, 1), ("msa col N=128 L=200", False, 4, 128, 200, 384, 12, 1)]
    shapes += [(f"floor sweep pair {ax} L={L}", True, 4, L, L, 288, 8, a_) for L in (16, 32, 48, 64) for ax, a_ in (("row", 1), ("col", 2))]
    for name, gen, B, L1, L2, D, H, axis in shapes:
        m = R.PerformerSelfAttention(dim=D, heads=H, generalized_attention=gen).cuda()
        iters = 5 if L1 >= 300 else 20 if L1 >= 100 else 200
        tf, tu = attend_ms(m, B, L1, L2, D, axis, True, iters), attend_ms(m, B, L1, L2, D, axis, False, iters)
        rows.append(dict(shape=name, B=B, L1=L1, L2=L2, D=D, H=H, axis=axis, fused_ms=tf, unfused_ms=tu, unfused_over_fused=tu / tf if tu else None))
        print(f"{name}: fused {tf*1e3:.0f} us, unfused " + (f"{tu*1e3:.0f} us, unfused / fused {tu/tf:.2f}" if tu else "refused (RF_EALIGN)"), flush=True)
    out = [a_ for a_ in sys.argv[1:] if a_.endswith(".json")]
    if out:
        json.dump(rows, open(out[0], "w"), indent=1)
    sys.exit(0)
for name, gen, B, L1, L2, D, H, axis in [("pair row", True, 4, 256, 256, 288, 8, 1), ("pair col", True, 4, 256, 256, 288, 8, 2), ("msa col", False, 4, 128, 256, 384, 12, 1)]:
    m = R.PerformerSelfAttention(dim=D, heads=H, generalized_attention=gen).cuda()
    inner = 64 * H
    qkv = torch.randn(B * L1 * L2, 3 * inner, device="cuda").bfloat16()
    o = torch.empty(B * L1 * L2, inner, device="cuda", dtype=torch.bfloat16)
    Ls, Lo = (L1, L2) if axis == 1 else (L2, L1)
    ss, so = (L2, 1) if axis == 1 else (1, L2)
    RB, W3 = L1 * L2, 3 * inner
    pc = m.proj_scaled(log2e=not gen)
    f = lambda: ops.favor_attention(qkv, pc, o, (RB * W3, so * W3, ss * W3, 64), (RB * inner, so * inner, ss * inner), 0, inner, 2 * inner, B, Lo, H, Ls, 64, 266, not gen, 1e-3 if gen else 1e-4)
    t = timeit(f)
    fl = B * Lo * H * (4 * 2 * Ls * 64 * 266)
    print(f"{name}: {t*1e3:.0f} us, {fl/t/1e9:.0f} TF/s (algorithmic, 266 features)", flush=True)
    # head-major q|k|v tiles: [Lo, 3H, B, Ls, 64] (every item's K / V / Q tile is one contiguous Ls x 128-byte block)
    qh = torch.randn(Lo, 3 * H, B, Ls, 64, device="cuda").bfloat16()
    fh = lambda: ops.favor_attention(qh, pc, o, (Ls * 64, 3 * H * B * Ls * 64, 64, B * Ls * 64), (RB * inner, so * inner, ss * inner), 0, H * B * Ls * 64, 2 * H * B * Ls * 64, B, Lo, H, Ls, 64, 266, not gen, 1e-3 if gen else 1e-4)
    t = timeit(fh)
    print(f"   head-major q|k|v tiles: {t*1e3:.0f} us, {fl/t/1e9:.0f} TF/s", flush=True)
    if int(os.environ.get("RF_FAVOR_DBG", "0")) & 8:
        import ctypes as C
        buf = (C.c_ulonglong * 7)()
        ops.lib.rf_favor_phase_cycles.argtypes = [C.c_void_p, C.c_int]
        ops.lib.rf_favor_phase_cycles(None, 1)
        f(); torch.cuda.synchronize()
        ops.lib.rf_favor_phase_cycles(buf, 1)
        n = max(buf[6], 1)
        names = ["wait K/V", "phase A", "publish + barrier", "prefetch issue + combine", "phase B", "stores"]
        print("   cycles per item (wave 0): " + ", ".join(f"{nm} {buf[i]/n:.0f}" for i, nm in enumerate(names)) + f"  [{n} items]")
