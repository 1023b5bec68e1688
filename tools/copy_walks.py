"""Which strided copies a tree issues, and whether two trees issue the same ones.

    copy_walks.py record  --tree DIR --out raw.json     run the scenarios below on the checkout at DIR (default: this one)
    copy_walks.py compare --parent a.json b.json --new c.json --out evidence.json

`record` hooks the C entry point rf_copy4d on both library handles (as bench.py wraps rf_gemm), so it works on any tree
whatever its Python copy wrapper looks like.  Per call it notes the two dtype codes, the raw (dims, xs, ys) the library received
and the Python call site: the first frame outside ops.py.  Per scenario it also writes the sha256 of every output and gradient.
`compare` puts every raw record through ops.copy_walk of THIS tree (dimensions of size 1 dropped, contiguous neighbours merged:
the sequence of addresses is unchanged) and checks: the two parent runs are identical (bit-reproducible), every scenario's
sequence of (dtype codes, walk) is equal between parent and new tree, every hash is equal; it lists how often each call site of
the parent ran.  Equal walks: the same kernel over the same addresses in the same order.  Equal hashes: every offset is right.

The row-sharded scenarios run two ranks on one GPU over gloo (as tests/test_rowshard_gpu.py does); rank 0's records count.
"""
import argparse
import hashlib
import json
import os
import sys
import tempfile
import traceback

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(d_input=21, d_msa=96, d_pair=72, d_node=8, d_edge=8, d_state=8, n_two_track_blocks=1, n_three_track_blocks=1,
           n_encoder_layers=1, max_len=64, n_neighbors=[16], p_dropout=0.0)
B, N, L = 2, 6, 20      # all distinct; map_ld(20) = 24 in the 16-bit modes
L8, N8 = 16, 8          # where a 16-bit mode takes whole 8-element pieces of a sequence or of the MSA depth (the shape of smoke())
HOST_ERRORS = (ValueError, TypeError, NotImplementedError, AssertionError, AttributeError, KeyError, IndexError)


# ------------------------------------------------------------------------------------------------ the hook
class Recorder:
    def __init__(self, tree):
        self.tree, self.calls = tree, []

    def install(self, _lib):
        for handle in _lib.LIBS.values():
            handle.rf_copy4d = self._wrap(handle.rf_copy4d)

    def _wrap(self, orig):
        def hooked(x, x_dt, xs, y, y_dt, ys, dims, stream):
            where = lambda fr: f"{os.path.relpath(fr.f_code.co_filename, self.tree)}:{fr.f_lineno}"  # noqa: E731
            f = sys._getframe(2)     # past the copy wrapper of ops.py
            via = where(f) if os.path.basename(f.f_code.co_filename) == "ops.py" else None   # a helper of ops.py that copies
            while f is not None and os.path.basename(f.f_code.co_filename) == "ops.py":
                f = f.f_back
            self.calls.append({"site": where(f) if f is not None else "?", "via": via, "dt": [int(x_dt), int(y_dt)],
                               "dims": list(dims._obj), "xs": list(xs._obj), "ys": list(ys._obj)})
            return orig(x, x_dt, xs, y, y_dt, ys, dims, stream)
        return hooked

    def take(self):
        out, self.calls = self.calls, []
        return out


def sha(t):
    import torch
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def hashes(named):
    return {k: sha(v) for k, v in sorted(named.items()) if v is not None}


# ------------------------------------------------------------------------------------------------ scenarios
def gen(seed):
    import torch
    return torch.Generator().manual_seed(seed)


def rn(*shape, seed=0, scale=1.0):
    import torch
    return (torch.randn(*shape, generator=gen(seed + len(shape) + sum(shape))) * scale).cuda()


def tokens(b=B, n=N, l=L):
    import torch
    msa = torch.randint(0, 21, (b, n, l), generator=gen(11))
    return msa.cuda(), msa[:, 0].clone().cuda(), torch.arange(l).unsqueeze(0).repeat(b, 1).cuda()


def grads_of(mod, inputs):
    out = {"p." + k: p.grad for k, p in mod.named_parameters()}
    out.update({f"in{i}": t.grad for i, t in enumerate(inputs) if t.requires_grad})
    return out


def coordinates(b, l, seed):
    import torch
    step = torch.randn(b, l, 3, generator=gen(7300 + seed))
    ca = (3.8 * step / step.norm(dim=-1, keepdim=True)).cumsum(1)
    return (ca[:, :, None, :] + 0.5 * torch.randn(b, l, 3, 3, generator=gen(7400 + seed))).float().contiguous().cuda()


def chain(dtype):
    import torch
    return L if dtype == torch.float32 else L8


def depth(dtype):
    import torch
    return N if dtype == torch.float32 else N8


def s_model_forward(R, dtype):
    import torch
    model = R.RoseTTAFold(**CFG).cuda().eval()
    with torch.no_grad():
        logits, xyz, plddt = model(*tokens(n=depth(dtype), l=chain(dtype)))
    return dict(logits, xyz=xyz, plddt=plddt)


def s_model_head_backward(R, dtype):
    """the trunk under no_grad, the head and the final block's axial update recording, dropout on"""
    import torch
    model = R.RoseTTAFold(**dict(CFG, p_dropout=0.1)).cuda().train()
    model.prediction_head.enable_backward()
    model.final_block.pair_update_with_axial_attention.enable_backward()
    logits, xyz, plddt = model(*tokens(n=N8, l=L8))
    sum((v * rn(*v.shape, seed=i)).sum() for i, (k, v) in enumerate(sorted(logits.items()))).backward()
    out = {"p." + k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    out.update(logits)
    return out


def tied(shape, train):
    def run(R, dtype):
        import torch
        b, n, l, d, h = shape
        mod = R.SoftTiedAttentionOverResidues(d, h, p_dropout=0.1 if train else 0.0, return_att=True).cuda()
        x = rn(b, n, l, d, seed=3)
        if not train:
            with torch.no_grad():
                out, att = mod.eval()(x)
            return {"out": out, "att": att}
        mod.train().enable_backward()
        x.requires_grad_()
        out, att = mod(x)
        ((out * rn(*out.shape, seed=4)).sum() + (att * rn(*att.shape, seed=5)).sum()).backward()
        return dict(grads_of(mod, [x]), out=out, att=att)
    return run


def s_poswise(R, dtype):
    mod = R.PositionWiseWeightFactor(16, 2, 0.1).cuda().train().enable_backward()
    x = rn(B, N, L, 16, seed=6).requires_grad_()
    out = mod(x)
    (out * rn(*out.shape, seed=7)).sum().backward()
    return dict(grads_of(mod, [x]), out=out)


def s_axial(R, dtype):
    mod = R.PairUpdateWithAxialAttentionLayer(32, 64, 2, 0.1, {}).cuda().train().enable_backward()
    x = rn(B, chain(dtype), chain(dtype), 32, seed=8).requires_grad_()
    out = mod(x)
    (out * rn(*out.shape, seed=9)).sum().backward()
    return dict(grads_of(mod, [x]), out=out)


def s_rowwise(R, dtype):
    import torch
    from rosettafold_pytorch_amd import model as M
    x = rn(B, N, L, 12, seed=10)
    return {"out": M.RowWise(torch.nn.Identity())(x)}


def s_symmetrization(R, dtype):
    return {"out": R.Symmetrization()(rn(B, L, L, 12, seed=12))}


def outer(p, dout, n, two):
    def run(R, dtype):
        mod = R.OuterProductMean(p, dout).cuda().enable_backward()
        x = rn(B, n, L, p, seed=13).requires_grad_()
        y = rn(B, n, L, p, seed=14).requires_grad_() if two else None
        out = mod(x, y) if two else mod(x)
        (out * rn(*out.shape, seed=15)).sum().backward()
        return dict(grads_of(mod, [x] + ([y] if two else [])), out=out)
    return run


def s_outer_fused_forward(R, dtype):
    import torch
    mod = R.OuterProductMean(32, 288).cuda().eval()
    with torch.no_grad():
        return {"out": mod(rn(B, N, L, 32, seed=16), rn(B, N, L, 32, seed=17))}


def s_outer_pad_depth(R, dtype):
    """operands handed over at a depth of 8: run() pads them to the fused kernel's 64 itself"""
    import torch
    from rosettafold_pytorch_amd import ops
    mod = R.OuterProductMean(32, 288).cuda().eval()
    with torch.no_grad():
        xt, yt, n8 = ops.outer_operands(rn(B, N, L, 32, seed=16), rn(B, N, L, 32, seed=17), dtype, 8)
        return {"out": mod.run(xt, yt, n8)}


def s_pair_update_with_msa(R, dtype):
    """d_feat = 2 * 24 + 4 * 8 + 3 = 83: the feature rows carry zero padding to 88"""
    import torch
    mod = R.PairUpdateWithMsa(32, 8, 24, 3, 0.0).cuda().eval()
    with torch.no_grad():
        return {"out": mod(rn(B, N, L, 32, seed=18), rn(B, L, L, 24, seed=19), rn(B, L, L, 3, seed=20))}


def s_msa_pair(R, dtype):
    mod = R.MsaUpdateWithPair(32, 24, 4, n_encoder_layers=2, p_dropout=0.1).cuda().train().enable_backward()
    m, p = rn(B, N, L, 32, seed=21).requires_grad_(), rn(B, L, L, 24, seed=22).requires_grad_()
    out = mod(m, p)
    (out * rn(*out.shape, seed=23)).sum().backward()
    return dict(grads_of(mod, [m, p]), out=out)


def s_initial_coord(R, dtype):
    import torch
    mod = R.InitialCoordGenerationWithMsaAndPair(24, 16, 8, 8, 4, 1, 0.1).cuda().train().enable_backward()
    m, p = rn(B, N, L, 24, seed=24).requires_grad_(), rn(B, L, L, 16, seed=25).requires_grad_()
    onehot = torch.nn.functional.one_hot(torch.randint(0, 21, (B, L), generator=gen(26)), 21).float().cuda()
    aa_idx = torch.arange(L).unsqueeze(0).repeat(B, 1)
    aa_idx[:, L // 2:] += 3
    out = mod(m, p, onehot, aa_idx.cuda())
    (out * rn(*out.shape, seed=27)).sum().backward()
    return dict(grads_of(mod, [m, p]), out=out)


def s_msa_coord(R, dtype):
    mod = R.MsaUpdateWithPairAndCoord(32, 16, 32, 128, p_dropout=0.1).cuda().train().enable_backward()
    st, m = rn(B, L, 16, seed=28).requires_grad_(), rn(B, N, L, 32, seed=29).requires_grad_()
    out = mod(coordinates(B, L, 2), st, m)
    (out * rn(*out.shape, seed=30)).sum().backward()
    return dict(grads_of(mod, [st, m]), out=out)


def s_head(R, dtype):
    mod = R.PredictionHead(32, 2, 0.15).cuda().train().enable_backward()
    x = rn(B, L, L, 32, seed=31).requires_grad_()
    outs = mod(x)
    sum((v * rn(*v.shape, seed=32 + i)).sum() for i, (k, v) in enumerate(sorted(outs.items()))).backward()
    return dict(grads_of(mod, [x]), **outs)


def s_pair_bias_attention(R, dtype):
    import torch
    from rosettafold_pytorch_amd import custom_ops  # noqa: F401
    h16 = torch.float16 if dtype == torch.float16 else torch.bfloat16
    return {"out": torch.ops.rfmi.pair_bias_attention(rn(B, L8, L8, 4, seed=40), rn(B, N, L8, 32, seed=41).to(h16),
                                                      rn(B, N, L8, 32, seed=42))}


def s_gathers_one_process(R, dtype):
    """the shard helpers without a process group: a world of one"""
    import torch
    from rosettafold_pytorch_amd import shard
    mod = R.MsaUpdateWithPair(32, 24, 4, n_encoder_layers=1, p_dropout=0.0).cuda().eval()
    with torch.no_grad():
        out = shard.msa_update_with_pair_row_sharded(mod, rn(B, N, L, 32, seed=43), rn(B, L, L, 24, seed=44))
        x = rn(B, L, 7, 12, seed=45)
        full = torch.zeros(B, N, L, 12, device="cuda")
        shard.all_gather_positions(rn(B, N, L, 12, seed=49), full)
        return {"msa": out, "full": full, "rows": shard.take_rows(x), "halo": shard.exchange_row_halos(rn(B, 5, 7, 8, seed=46), 2),
                "cut": shard.drop_row_halos(rn(B, 9, 7, 8, seed=47), 2), "t": shard.transpose_row_sharded(rn(B, 7, 7, 5, seed=48))}


# ---- two ranks on one GPU (gloo)
def w_forward(R, dtype):
    import torch
    from rosettafold_pytorch_amd import shard
    model = R.RoseTTAFold(**dict(CFG, n_three_track_blocks=2, n_neighbors=[16, 16])).cuda().eval()
    with torch.no_grad():
        logits, xyz, plddt = shard.forward_row_sharded(model, *[t.cpu() for t in tokens(1, N + 2, L + 12)])
    return dict(logits, xyz=xyz, plddt=plddt)


def w_two_track(R, dtype):
    """two samples: the convolutions take the exchanged-halo route, not the pre-haloed one-picture buffers"""
    import torch
    import torch.distributed as dist
    from rosettafold_pytorch_amd import shard
    blk = R.TwoTrackBlock(96, 72, 1, 0.0).cuda().eval()
    l = chain(dtype)
    r0, r1 = shard.shard_range(l, 2, dist.get_rank())
    with torch.no_grad():
        m, p = shard.two_track_block_row_sharded(blk, rn(B, depth(dtype), l, 96, seed=50), rn(B, l, l, 72, seed=51)[:, r0:r1].contiguous())
    return {"msa": m, "pair": p}


def w_head(R, dtype):
    import torch
    import torch.distributed as dist
    from rosettafold_pytorch_amd import shard
    head = R.PredictionHead(32, 2, 0.0).cuda().eval()
    r0, r1 = shard.shard_range(L, 2, dist.get_rank())
    with torch.no_grad():
        return dict(shard.prediction_head_row_sharded(head, rn(B, L, L, 32, seed=52)[:, r0:r1].contiguous()))


F32, BF16, F16 = "float32", "bfloat16", "float16"
SCENARIOS = [   # (name, function, compute dtypes)
    ("model_forward", s_model_forward, (F32, BF16, F16)),
    ("model_head_backward", s_model_head_backward, (BF16,)),
    ("tied_general_train", tied((2, 3, 20, 32, 2), True), (F32, BF16, F16)),
    ("tied_head_major_train", tied((1, 4, 63, 96, 3), True), (BF16, F16)),
    ("tied_head_major", tied((1, 4, 63, 96, 3), False), (BF16,)),
    ("tied_fused_logits", tied((1, 3, 64, 96, 3), False), (BF16,)),
    ("tied_long_rows", tied((1, 64, 257, 384, 12), False), (BF16,)),
    ("poswise", s_poswise, (F32, BF16)),
    ("axial_layer", s_axial, (F32, BF16, F16)),
    ("rowwise", s_rowwise, (F32,)),
    ("symmetrization", s_symmetrization, (F32,)),
    ("outer_general_two", outer(4, 16, N, True), (F32, BF16, F16)),
    ("outer_general_one", outer(8, 16, N + 3, False), (BF16,)),
    ("outer_fused_forward", s_outer_fused_forward, (BF16, F16)),
    ("outer_pad_depth", s_outer_pad_depth, (BF16,)),
    ("pair_update_with_msa", s_pair_update_with_msa, (F32, BF16)),
    ("msa_pair", s_msa_pair, (F32, BF16, F16)),
    ("initial_coord", s_initial_coord, (F32, BF16)),
    ("msa_coord", s_msa_coord, (F32, BF16)),
    ("head", s_head, (F32, BF16)),
    ("pair_bias_attention", s_pair_bias_attention, (BF16, F16)),
    ("gathers_one_process", s_gathers_one_process, (F32,)),
]
WORLD2 = [
    ("world2_forward", w_forward, (F32, BF16)),
    ("world2_two_track", w_two_track, (F32, BF16)),
    ("world2_head", w_head, (BF16,)),
]


def run_list(R, rec, scenarios, result):
    """-> False when a scenario ended in anything but a host-side refusal: nothing more is started on the GPU then"""
    import torch
    for name, fn, dtypes in scenarios:
        for dt in dtypes:
            key = f"{name}/{dt}"
            R.set_compute_dtype(getattr(torch, dt))
            torch.manual_seed(1234)
            rec.take()
            try:
                out = fn(R, getattr(torch, dt))
                torch.cuda.synchronize()
                result[key] = {"calls": rec.take(), "hashes": hashes(out)}
            except Exception as e:
                result[key] = {"calls": rec.take(), "error": traceback.format_exc(limit=-3)}
                refused = isinstance(e, HOST_ERRORS) or (type(e).__name__ == "RfmiError" and "hipError_t" not in str(e))
                if not refused:   # anything the device may have had a part in
                    return False
            finally:
                R.set_compute_dtype(torch.bfloat16)
    return True


def _rank(rank, port, tree, out):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, tree)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=2)
    import rosettafold_pytorch_amd as R
    from rosettafold_pytorch_amd import _lib
    rec = Recorder(tree)
    rec.install(_lib)
    result = {}
    ok = run_list(R, rec, WORLD2, result)
    if rank == 0:
        with open(out, "w") as f:
            json.dump(result, f)
    if ok:
        dist.barrier()
        dist.destroy_process_group()
    sys.exit(0 if ok else 3)


def record(args):
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    import torch
    import torch.multiprocessing as mp
    import rosettafold_pytorch_amd as R
    from rosettafold_pytorch_amd import _lib
    assert os.path.abspath(R.__path__[0]).startswith(tree), R.__path__
    torch.cuda.set_device(0)
    rec = Recorder(tree)
    rec.install(_lib)
    result = {}
    ok = run_list(R, rec, SCENARIOS, result)
    if ok and not args.no_world2:
        with tempfile.TemporaryDirectory() as tmp:
            part = os.path.join(tmp, "w2.json")
            ctx = mp.get_context("spawn")
            procs = [ctx.Process(target=_rank, args=(r, 47100 + os.getpid() % 2000, tree, part)) for r in range(2)]
            for p in procs:
                p.start()
            for p in procs:
                p.join(300)
            ok = all(p.exitcode == 0 for p in procs)
            for p in procs:
                if p.is_alive():
                    p.kill()
            if os.path.exists(part):
                result.update(json.load(open(part)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tree": args.label or tree, "scenarios": result}, f, indent=1)
    errors = {k: v["error"] for k, v in result.items() if "error" in v}
    sites = {}
    for v in result.values():
        for c in v["calls"]:
            sites[c["via"] or c["site"]] = sites.get(c["via"] or c["site"], 0) + 1
    print(json.dumps({"scenarios": len(result), "errors": errors, "sites": len(sites), "calls": sum(sites.values())}, indent=1))
    for s in sorted(sites):
        print(f"{sites[s]:6d}  {s}")
    return 0 if ok and not errors else 1


# ------------------------------------------------------------------------------------------------ compare
def walks(calls):
    sys.path.insert(0, HERE)
    from rosettafold_pytorch_amd import ops
    return [[c["dt"], [list(t) for t in ops.copy_walk(c["dims"], c["xs"], c["ys"])]] for c in calls]


def compare(args):
    pa, pb, new = (json.load(open(p))["scenarios"] for p in (*args.parent, args.new))
    sites, rows, failures = {}, {}, []
    for key, a in pa.items():
        for c in a["calls"]:
            sites[c["via"] or c["site"]] = sites.get(c["via"] or c["site"], 0) + 1
        b, n = pb.get(key), new.get(key)
        last = [v["error"].strip().splitlines()[-1] if v is not None and "error" in v else None for v in (a, b, n)]
        if last[0] is not None and last[0] == last[1] == last[2]:   # refused alike by every tree before any result: no evidence
            rows[key] = {"refused_by_every_tree": last[0][:160]}
            continue
        if b is None or n is None or any("error" in v for v in (a, b, n)):
            failures.append(f"{key}: missing or failed in one of the runs")
            continue
        a, b, n = ({"calls": [{k: c[k] for k in ("dt", "dims", "xs", "ys")} for c in v["calls"]], "hashes": v["hashes"]}
                   for v in (a, b, n))
        wa, wn = walks(a["calls"]), walks(n["calls"])
        row = {"copies": len(wa), "parent_reproducible": a == b, "walks_equal": wa == wn, "hashes_equal": a["hashes"] == n["hashes"],
               "outputs": len(a["hashes"])}
        rows[key] = row
        failures += [f"{key}: {k}" for k in ("parent_reproducible", "walks_equal", "hashes_equal") if not row[k]]
        if not row["walks_equal"]:
            for i, (x, y) in enumerate(zip(wa, wn)):
                if x != y:
                    failures.append(f"{key}: copy {i} at {pa[key]['calls'][i]['site']}: parent {x}, new {y}")
                    break
        if not row["hashes_equal"]:
            failures.append(f"{key}: differing {sorted(k for k in a['hashes'] if a['hashes'][k] != n['hashes'].get(k))[:6]}")
    out = {"what": "tools/copy_walks.py: every rf_copy4d call of a fixed list of seeded scenarios, parent tree (run twice) and new tree",
           "parent_call_sites": len(sites), "parent_site_runs": dict(sorted(sites.items())), "scenarios": rows,
           "all_parent_reproducible": all(r.get("parent_reproducible", True) for r in rows.values()),
           "all_walks_equal": all(r.get("walks_equal", True) for r in rows.values()),
           "all_hashes_equal": all(r.get("hashes_equal", True) for r in rows.values()), "failures": failures}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k not in ("scenarios", "parent_site_runs")}, indent=1))
    return 1 if failures else 0


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("record")
    r.add_argument("--tree", default=HERE)
    r.add_argument("--label", default=None)
    r.add_argument("--out", required=True)
    r.add_argument("--no-world2", action="store_true")
    c = sub.add_parser("compare")
    c.add_argument("--parent", nargs=2, required=True)
    c.add_argument("--new", required=True)
    c.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.exit(record(args) if args.cmd == "record" else compare(args))


if __name__ == "__main__":
    main()
