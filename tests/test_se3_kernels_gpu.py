"""Every kernel of csrc/se3.hip on its own against the float64 form of the CPU oracle (oracle/rf_oracle.py), on ragged graphs
built from hand-made masks (degrees a kNN rule never produces: empty rows, full rows, isolated nodes, self loops).

Tolerance.  Nothing here is a fixed number.  Every comparison evaluates the oracle twice on the kernel's own inputs, in
float64 (the reference) and in float32, and forms e32 = error of the float32 oracle against the float64 one -- the reference
measuring itself.  The kernel's error against float64 must stay within 8 * e32: the kernels sum in another order, use rsqrtf /
__expf and contract FMAs, a few more roundings than ATen; a wrong row order, a dropped bias or a lost edge is five or more orders
above that.  Two metrics, both over every valid element (the only rows left out are the documented tail rows past count[0]):
  l2   ||got - ref|| / ||ref||
  row  max over rows of ||got_r - ref_r|| / rms_r ||ref_r||      (one wrong edge among thousands cannot hide in the l2)
Integer outputs and stated zeros are exact.  Every comparison prints one `[se3]` line: kernel error, e32 and their ratio.

Graphs come from a uint8 mask through ops.edges_from_mask and ops.se3_edge_geometry (not build_graph); torch.where(mask) is the
reference edge list in the same row-major order.  Weights come from the product's own modules under a fixed seed, with the
LayerNorm gains / biases and the radial nets' last biases randomised (a swapped gamma / beta or a dropped bias shows); the
oracle's parameter dict is the module's state_dict cast to double."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import ops, structure as S  # noqa: E402
from oracle import rf_oracle as O  # noqa: E402

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
FACTOR = 8.0


# ------------------------------------------------------------------------------------------------ comparison
def _rows(t):
    t = t.detach().cpu().double()
    return t.reshape(t.shape[0], -1) if t.dim() > 1 else t.reshape(-1, 1)


def _errors(a, ref):
    d = (a - ref).norm(dim=1)
    rn_ = ref.norm(dim=1)
    return (d.norm() / ref.norm()).item(), (d.max() / rn_.pow(2).mean().sqrt()).item()


def compare(name, got, ref64, ref32):
    """got: the kernel's result; ref64 / ref32: the oracle on the same inputs in float64 / float32 (first dim = rows)."""
    got, ref64, ref32 = _rows(got), _rows(ref64), _rows(ref32)
    assert got.shape == ref64.shape == ref32.shape, (name, got.shape, ref64.shape, ref32.shape)
    assert torch.isfinite(ref64).all(), name   # the inputs are chosen so that the reference is finite everywhere
    assert torch.isfinite(got).all(), name
    assert ref64.norm() > 0, name
    (k2, kr), (o2, orow) = _errors(got, ref64), _errors(ref32, ref64)
    line = (f"[se3] {name}: l2 kernel {k2:.3e} e32 {o2:.3e} ratio {k2 / o2 if o2 else float(k2 > 0):.2f} | "
            f"row kernel {kr:.3e} e32 {orow:.3e} ratio {kr / orow if orow else float(kr > 0):.2f}")
    print(line)
    assert k2 <= FACTOR * o2 and kr <= FACTOR * orow, line


# ------------------------------------------------------------------------------------------------ inputs
def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(*s, seed):
    return torch.randn(*s, generator=gen(seed))


def chain(b, l, seed=3):
    """random-walk CA trace with N / C around it, [b, l, 3, 3] fp32 (|xyz| grows to tens of angstroms)"""
    g = gen(seed)
    steps = torch.randn(b, l, 3, generator=g)
    ca = torch.cumsum(3.8 * steps / steps.norm(dim=-1, keepdim=True), 1)
    xyz = ca[:, :, None, :] + 0.5 * torch.randn(b, l, 3, 3, generator=g)
    xyz[:, :, 1] = ca
    return xyz


def ceil64(n):
    return max(64, (n + 63) // 64 * 64)


def trim(mask, n):
    """the mask with only its first n edges (row-major) kept"""
    flat = mask.reshape(-1).clone()
    on = flat.nonzero().reshape(-1)
    assert on.numel() >= n
    flat[on[n:]] = 0
    return flat.view_as(mask)


def edge_list(mask):
    b, i, j = torch.where(mask.bool())
    L_ = mask.shape[1]
    return b * L_ + i, b * L_ + j


def device_edges(mask, cap):
    src, dst, eid, count = ops.edges_from_mask(mask.to(DEV).contiguous(), cap, zero_tail=True)
    n = int(mask.sum())
    assert count.tolist() == [n, n]
    return src, dst, eid, count


def device_graph(mask, xyz, edge_emb, cap=None):
    """the graph dict GSE3Res.run reads (structure.build_graph's keys) from a hand-made mask"""
    B, L_ = mask.shape[:2]
    n = int(mask.sum())
    cap = cap or ceil64(n)
    src, dst, eid, count = device_edges(mask, cap)
    basis, feat = ops.se3_edge_geometry(xyz.to(DEV).contiguous(), edge_emb.to(DEV).contiguous(), src, dst, count, cap)
    return {"src": src, "dst": dst, "eid": eid, "count": count, "basis": basis, "feat": feat, "cap": cap, "V": B * L_,
            "L": L_, "n": n}


def basis_dict(basis, dtype):
    """the 34 floats per edge (layout at RF_BASIS_LD, csrc/se3.hip) as the oracle's basis[(d_in, d_out)] [E, 2do+1, 2di+1, nJ]"""
    b = basis.detach().cpu().to(dtype)
    n = b.shape[0]
    return {(0, 0): b[:, 0:1].reshape(n, 1, 1, 1), (0, 1): b[:, 1:4].reshape(n, 3, 1, 1),
            (1, 0): b[:, 4:7].reshape(n, 1, 3, 1), (1, 1): b[:, 7:34].reshape(n, 3, 3, 3)}


def basis_rows(bd):
    """the oracle's basis dict as [E, 34] rows in the kernel's layout"""
    n = bd[(0, 0)].shape[0]
    return torch.cat([bd[(0, 0)].reshape(n, 1), bd[(0, 1)].reshape(n, 3), bd[(1, 0)].reshape(n, 3), bd[(1, 1)].reshape(n, 27)], 1)


def build(ctor, seed):
    """the product's module under a fixed seed; LayerNorm gains / biases and the radial nets' last biases moved off 1 / 0"""
    torch.manual_seed(seed)
    m = ctor()
    g = gen(seed + 1000)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.LayerNorm):
                mod.weight.copy_(1.0 + 0.3 * torch.randn(mod.weight.shape, generator=g))
                mod.bias.copy_(0.3 * torch.randn(mod.bias.shape, generator=g))
            if isinstance(mod, S.RadialFunc):
                mod.net[6].bias.copy_(0.3 * torch.randn(mod.net[6].bias.shape, generator=g))
    return m.to(DEV).eval()


def params(m, dtype):
    return {"m." + k: v.detach().cpu().to(dtype) for k, v in m.state_dict().items()}


def node_features(V, mi0, mi1, seed):
    """h0 [V, mi0, 1], h1 [V, mi1, 3] fp32 with a few exact zeros (None for an absent degree)"""
    h0 = randn(V, mi0, 1, seed=seed) if mi0 else None
    h1 = randn(V, mi1, 3, seed=seed + 1) if mi1 else None
    for h in (h0, h1):
        if h is not None:
            h.view(-1)[::37] = 0.0
            h[V // 2] = 0.0
    return h0, h1


def to_dev(t):
    return None if t is None else t.to(DEV).contiguous()


# ------------------------------------------------------------------------------------------------ 0. kNN mask
@pytest.mark.parametrize("k", [4, 32, 200])
def test_knn_mask(k):
    """rf_knn_mask against the oracle's rule (k nearest or |idx_i - idx_j| < kmin) on a chain with a break; k >= L keeps the
    self loop.  Integer work: exact."""
    B, L_ = 2, 70
    xyz = chain(B, L_, seed=11)
    aa = torch.arange(L_).repeat(B, 1)
    aa[1, 40:] += 200
    mask = ops.knn_mask(xyz.to(DEV), aa.to(DEV), k, 9).cpu()
    want = torch.zeros(B, L_, L_, dtype=torch.uint8)
    want[O.knn_graph(xyz, aa, k)] = 1
    assert torch.equal(mask, want)
    one = ops.knn_mask(xyz[:1, :1].contiguous().to(DEV), aa[:1, :1].contiguous().to(DEV), k, 9).cpu()
    assert one.tolist() == [[[1]]]      # L = 1: k >= L, the node is its own nearest neighbour


# ------------------------------------------------------------------------------------------------ 1. edge compaction
def compaction_mask(B, L_, seed):
    m = (torch.rand(B, L_, L_, generator=gen(seed)) < 0.3).to(torch.uint8)
    for r in range(0, L_, 17):
        m[:, r, r] = 1            # the diagonal on a few rows
    if L_ >= 4:
        m[:, 1, :] = 0            # an empty row
        m[:, 2, :] = 1            # a full row
        m[:, :, 3] = 0            # an empty column (also in the full row)
    return m


@pytest.mark.parametrize("B,L_", [(1, 1), (2, 70), (2, 257), (1, 300)])
@pytest.mark.parametrize("kind", ["random", "zero"])
def test_edges_from_mask(B, L_, kind):
    mask = compaction_mask(B, L_, seed=L_) if kind == "random" else torch.zeros(B, L_, L_, dtype=torch.uint8)
    b, i, j = torch.where(mask.bool())
    n = b.numel()
    assert (n > 0) == (kind == "random")
    want_eid = torch.full((B, L_, L_), -1, dtype=torch.int32)
    want_eid[b, i, j] = torch.arange(n, dtype=torch.int32)
    # capacities: exactly the edge count, and the count rounded up to 64 (an empty list still needs one slot: capacity 0 is invalid)
    for cap in (max(n, 1), ceil64(n)):
        src, dst, eid, count = ops.edges_from_mask(mask.to(DEV), cap, zero_tail=True)
        assert count.tolist() == [n, n], (cap, count.tolist())
        assert torch.equal(src[:n].cpu().long(), b * L_ + i) and torch.equal(dst[:n].cpu().long(), b * L_ + j), cap
        assert torch.equal(eid.cpu(), want_eid), cap
        assert not src[n:].any() and not dst[n:].any(), cap   # the zeroed tail is never written


# ------------------------------------------------------------------------------------------------ 2. edge geometry
def geometry_case():
    """B = 2, L = 70.  Sample 0: node 0 at integer coordinates, nodes 1..6 on its +-x, +-y, +-z axes at integer distances, the
    others at distances 1e-3 .. 1e3 from it; node 0 points to every node (itself included: a zero-length edge) and every node
    points back.  Sample 1: a random-walk chain under a p = 0.3 mask.  A few more self loops in both."""
    B, L_, de = 2, 70, 8
    g = gen(21)
    xyz = chain(B, L_, seed=5)
    c0 = torch.tensor([1.0, 2.0, 3.0])
    ca = torch.empty(L_, 3)
    ca[0] = c0
    axes = torch.tensor([[3.0, 0, 0], [-2.0, 0, 0], [0, 5.0, 0], [0, -1.0, 0], [0, 0, 4.0], [0, 0, -7.0]])
    ca[1:7] = c0 + axes
    u = torch.rand(L_ - 7, generator=g) * 6.0 - 3.0
    u[0], u[1] = -3.0, 3.0
    dirs = torch.randn(L_ - 7, 3, generator=g)
    ca[7:] = c0 + dirs / dirs.norm(dim=-1, keepdim=True) * (10.0 ** u)[:, None]
    xyz[0, :, 1] = ca
    mask = (torch.rand(B, L_, L_, generator=g) < torch.tensor([0.1, 0.3])[:, None, None]).to(torch.uint8)
    mask[0, 0, :] = 1
    mask[0, :, 0] = 1
    for r in (0, 9, 33, 69):
        mask[:, r, r] = 1
    edge = torch.randn(B, L_, L_, de, generator=g)
    return mask, xyz, edge


def test_edge_geometry():
    mask, xyz, edge = geometry_case()
    B, L_, de = 2, 70, edge.shape[-1]
    src, dst = edge_list(mask)
    n = src.numel()
    gr = device_graph(mask, xyz, edge, cap=ceil64(n) + 64)
    ca = xyz[:, :, 1].reshape(-1, 3)
    d32 = ca[dst] - ca[src]
    d64 = ca.double()[dst] - ca.double()[src]
    r64 = d64.norm(dim=-1)
    assert (r64 == 0).sum() >= 8 and r64[r64 > 0].min() < 2e-3 and r64.max() > 5e2   # zero-length edges; lengths 1e-3 .. 1e3
    basis, feat = gr["basis"].cpu(), gr["feat"].cpu()
    assert not basis[n:].any() and not feat[n:].any()                  # rows at and past count[0]: exactly 0
    compare("edge_geometry basis", basis[:n], basis_rows(O.se3_basis(d64)), basis_rows(O.se3_basis(d32)))
    w = edge.reshape(-1, L_, de)[src, dst % L_]                         # edge_emb[b, i, j]
    assert torch.equal(feat[:n, :de], w)                                # the gathered embedding is a copy
    compare("edge_geometry feat [w | r]", feat[:n], torch.cat([w.double(), r64[:, None]], 1),
            torch.cat([w, d32.norm(dim=-1, keepdim=True)], 1))
    compare("edge_geometry r", feat[:n, de], r64, d32.norm(dim=-1))


# ------------------------------------------------------------------------------------------------ 3. fused radial message
NFULL = 700


@functools.lru_cache(maxsize=None)
def message_case(de):
    """B = 2, L = 70 chain under a sparse random mask (>= 700 edges, sources repeat, both samples reached by the first 700), one
    self loop (a zero-length edge) among the first 257 edges."""
    B, L_ = 2, 70
    mask = (torch.rand(B, L_, L_, generator=gen(31)) < 0.08).to(torch.uint8)
    mask[0, 3, 3] = 1
    assert int(mask[0].sum()) < NFULL <= int(mask.sum())
    return mask, chain(B, L_, seed=7), randn(B, L_, L_, de, seed=32)


@functools.lru_cache(maxsize=None)
def message_graph(de, n, cap):
    """the first n edges of message_case(de) as a device graph (shared by the tests: never modified, poison goes into clones)"""
    mask, xyz, edge = message_case(de)
    return device_graph(trim(mask, n), xyz, edge, cap)


def message_reference(conv, f_in, f_out, h, gr):
    """O.gconv_partial on the device graph's own feat / basis / src, in float64 and float32 -> ({dout: ref64}, {dout: ref32})"""
    n = gr["n"]
    src = gr["src"][:n].cpu().long()
    out = []
    for dt in (F64, F32):
        hh = {d: v.to(dt) for d, v in h.items() if v is not None}
        out.append(O.gconv_partial(params(conv, dt), "m", hh, f_in, f_out, gr["feat"][:n].cpu().to(dt),
                                   basis_dict(gr["basis"][:n], dt), src))
    return out


COUNTS_ALL = [(1, 64), (255, 256), (256, 256), (257, 320), (511, 512), (512, 512), (513, 576), (700, 704), (300, 1600)]
COUNTS_FEW = [(257, 320), (700, 704)]
FUSED = [  # (mo, dout, mi0, mi1, d_edge, (n, capacity) list)
    (4, 0, 8, 3, 8, COUNTS_ALL), (4, 1, 8, 3, 8, COUNTS_FEW),                       # layer 0
    (4, 0, 16, 16, 8, COUNTS_FEW), (4, 1, 16, 16, 8, COUNTS_ALL),                   # layer 2
    (3, 1, 16, 16, 8, COUNTS_ALL), (8, 0, 16, 16, 8, COUNTS_FEW), (16, 0, 16, 16, 8, COUNTS_ALL), (32, 0, 16, 16, 8, COUNTS_FEW),
    (32, 0, 16, 16, 64, COUNTS_FEW), (4, 1, 64, 3, 64, COUNTS_FEW),                 # production widths (the first: > 64 KB of LDS)
    (4, 0, 16, 0, 8, COUNTS_FEW), (4, 1, 0, 16, 8, COUNTS_FEW),                     # one-input forms of the C ABI
]


@pytest.mark.parametrize("mo,dout,mi0,mi1,de,counts", FUSED, ids=[f"mo{c[0]}-dout{c[1]}-mi{c[2]}_{c[3]}-ki{c[4] + 1}" for c in FUSED])
def test_fused_radial_message(mo, dout, mi0, mi1, de, counts):
    ki = de + 1
    assert ops.se3_radial_message_supported(mo, dout, mi0, mi1, ki)
    f_in = {d: m for d, m in ((0, mi0), (1, mi1)) if m}
    conv = build(lambda: S.GConvSE3Partial(f_in, {dout: mo}, edge_dim=de), seed=40 + mo + dout)
    net = {d: S._pack_radial_net(conv.kernel_unary[f"({d},{dout})"].rp) for d in f_in}
    full = message_graph(de, NFULL, ceil64(NFULL))
    V = full["V"]
    h0, h1 = node_features(V, mi0, mi1, seed=50)
    ref64, ref32 = message_reference(conv, f_in, {dout: mo}, {0: h0, 1: h1}, full)
    eps = conv.kernel_unary[f"({min(f_in)},{dout})"].rp.net[1].bn.eps
    for n, cap in counts:
        gr = message_graph(de, n, cap)
        assert gr["count"].tolist() == [n, n]                               # what edges_from_mask wrote
        assert torch.equal(gr["feat"][:n], full["feat"][:n]) and torch.equal(gr["basis"][:n], full["basis"][:n])
        feat, basis, src = gr["feat"].clone(), gr["basis"].clone(), gr["src"].clone()
        feat[n:] = float("nan")      # the tails are never read: NaN there must not reach a valid row ...
        basis[n:] = float("nan")
        src[n:] = V - 1              # ... and a (valid, non-zero) tail source must not be gathered into a stored row
        msg = ops.se3_radial_message(feat, ki, net.get(0), net.get(1), basis, to_dev(h0), to_dev(h1), src, gr["count"], mo, dout,
                                     mi0, mi1, eps, cap, zero_tail=True).cpu()
        assert msg.shape == (cap, mo, 2 * dout + 1)
        assert not msg[n:].any(), (n, cap)            # rows at and past n: still exactly 0
        assert not torch.isnan(msg[:n]).any(), (n, cap)
        compare(f"fused_radial_message mo={mo} dout={dout} mi=({mi0},{mi1}) ki={ki} n={n} cap={cap}", msg[:n],
                ref64[dout][:n], ref32[dout][:n])


# ------------------------------------------------------------------------------------------------ 4a. unfused message kernel
@pytest.mark.parametrize("dout", [0, 1])
@pytest.mark.parametrize("mo,mi0,mi1", [(4, 8, 3), (3, 16, 16), (12, 16, 16)])
def test_se3_message(mo, mi0, mi1, dout):
    """ops.se3_message alone: the radial outputs R come from O.radial_func in float64, rounded to float32."""
    de = 8
    f_in = {0: mi0, 1: mi1}
    conv = build(lambda: S.GConvSE3Partial(f_in, {dout: mo}, edge_dim=de), seed=60 + mo + dout)
    full = message_graph(de, NFULL, ceil64(NFULL))
    h0, h1 = node_features(full["V"], mi0, mi1, seed=61)
    ref64, ref32 = message_reference(conv, f_in, {dout: mo}, {0: h0, 1: h1}, full)
    P64 = params(conv, F64)
    Rfull = [O.radial_func(P64, f"m.kernel_unary.({di},{dout}).rp", full["feat"][:NFULL].cpu().double()).float() for di in (0, 1)]
    for n, cap in COUNTS_FEW:
        gr = message_graph(de, n, cap)
        Rn = []
        for r in Rfull:
            pad = torch.zeros(cap, r.shape[1])
            pad[:n] = r[:n]
            Rn.append(pad.to(DEV))
        msg = ops.se3_message(Rn[0], Rn[1], gr["basis"], to_dev(h0), to_dev(h1), gr["src"], gr["count"], mo, dout, mi0, mi1, cap).cpu()
        compare(f"se3_message mo={mo} dout={dout} mi=({mi0},{mi1}) n={n}", msg[:n], ref64[dout][:n], ref32[dout][:n])


# ------------------------------------------------------------------------------------------------ 4b. GSE3Res, both routes
@functools.lru_cache(maxsize=None)
def res_graph():
    """B = 2, L = 70, p = 0.3: node 5 of sample 0 is isolated (no edge in or out), every other node of sample 1 points to its
    node 7; one self loop."""
    B, L_, de = 2, 70, 8
    mask = (torch.rand(B, L_, L_, generator=gen(71)) < 0.3).to(torch.uint8)
    mask[0, 5, :] = 0
    mask[0, :, 5] = 0
    mask[1, :, 7] = 1
    mask[1, 7, 7] = 0
    mask[0, 11, 11] = 1
    return mask, device_graph(mask, chain(B, L_, seed=9), randn(B, L_, L_, de, seed=72))


RES = [(ds, "layer4") for ds in (8, 16, 32, 12)] + [(16, "layer0")]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("d_state,layer", RES, ids=[f"{l}-{d}" for d, l in RES])
def test_gse3res_routes(d_state, layer, fused):
    """GSE3Res.run against O.gse3res with runtime.se3_fused_radial on and off: the fused kernels, the launch chain (layer-1 GEMM,
    grouped LayerNorm, strided 32x32 GEMMs, last-layer GEMMs, ops.se3_message) and, at d_state = 12, both in one call (no fused
    degree-0 instance for 12 channels).  Each route meets the ceiling against float64 on its own."""
    if layer == "layer4":
        f_in, f_out, div, heads, si = {0: 16, 1: 16}, {0: d_state, 1: 3}, 1, 1, "att"
    else:
        f_in, f_out, div, heads, si = {0: 8, 1: 3}, {0: 16, 1: 16}, 4, 4, "1x1"
    mask, gr = res_graph()
    src, dst = edge_list(mask)
    n, V = gr["n"], gr["V"]
    mod = build(lambda: S.GSE3Res(f_in, f_out, edge_dim=8, div=div, n_heads=heads, selfint=si), seed=80 + d_state)
    h0, h1 = node_features(V, f_in[0], f_in[1], seed=81)
    mixed = [ops.se3_radial_message_supported(m, d, f_in[0], f_in[1], 9) for d, m in mod.f_mid_out.items()]
    assert all(mixed) == (d_state != 12) and any(mixed)
    was = R.RT.se3_fused_radial
    R.RT.se3_fused_radial = fused
    try:
        out = mod.run({0: to_dev(h0), 1: to_dev(h1)}, gr)
    finally:
        R.RT.se3_fused_radial = was
    ref = []
    for dt in (F64, F32):
        ref.append(O.gse3res(params(mod, dt), "m", {0: h0.to(dt), 1: h1.to(dt)}, f_in, f_out, div, heads, si,
                             gr["feat"][:n].cpu().to(dt), basis_dict(gr["basis"][:n], dt), src, dst, V))
    for d in (0, 1):
        assert out[d].shape == (V, f_out[d], 2 * d + 1)
        compare(f"gse3res {layer} d_state={d_state} {'fused' if fused else 'unfused'} degree {d}", out[d], ref[0][d], ref[1][d])


# ------------------------------------------------------------------------------------------------ 5. graph attention
def attention_mask(B, L_, seed):
    """p = 0.3; node 0 has no incoming edge, node 1 exactly one, node 2 one from every node (itself included)"""
    if L_ == 1:
        return torch.ones(B, 1, 1, dtype=torch.uint8)
    mask = (torch.rand(B, L_, L_, generator=gen(seed)) < 0.3).to(torch.uint8)
    mask[:, :, 0] = 0
    mask[:, :, 1] = 0
    mask[:, L_ // 2, 1] = 1
    mask[:, :, 2] = 1
    return mask


HEADS = [(4, 4, 4, 4, 4), (1, 16, 3, 16, 3), (1, 12, 3, 12, 3), (1, 32, 3, 32, 3)]   # (heads, mk0, mk1, mv0, mv1)


def attention_inputs(mask, heads, mk0, mk1, mv0, mv1, seed, q_scale=1.0, equal=False):
    B, L_ = mask.shape[:2]
    n, V = int(mask.sum()), B * L_
    k = {0: randn(n, mk0, 1, seed=seed), 1: randn(n, mk1, 3, seed=seed + 1)}
    v = {0: randn(n, mv0, 1, seed=seed + 2), 1: randn(n, mv1, 3, seed=seed + 3)}
    q = {0: q_scale * randn(V, mk0, 1, seed=seed + 4), 1: q_scale * randn(V, mk1, 3, seed=seed + 5)}
    if equal:   # the same key on every edge: all logits of a node are equal (and not zero)
        k = {d: t[:1].expand_as(t).contiguous() for d, t in k.items()}
    return k, q, v


def run_attention(mask, k, q, v, heads, skip=None):
    B, L_ = mask.shape[:2]
    n, V = int(mask.sum()), B * L_
    cap = ceil64(n)
    _, _, eid, _ = device_edges(mask, cap)

    def edges(t):   # [n, m, c] -> device [cap, m, c]
        pad = torch.zeros(cap, *t.shape[1:])
        pad[:n] = t[:n]
        return pad.to(DEV)
    s0, s1 = (to_dev(skip[0]), to_dev(skip[1])) if skip else (None, None)
    return ops.se3_attention(edges(k[0]), edges(k[1]), to_dev(q[0]), to_dev(q[1]), edges(v[0]), edges(v[1]), eid, heads,
                             k[0].shape[1], k[1].shape[1], v[0].shape[1], v[1].shape[1], V, L_, skip0=s0, skip1=s1)


def attention_reference(mask, k, q, v, heads):
    src, dst = edge_list(mask)
    V = mask.shape[0] * mask.shape[1]
    ref = []
    for dt in (F64, F32):
        c = lambda t: {d: x.to(dt) for d, x in t.items()}  # noqa: E731
        ref.append(O.gmab(c(v), c(k), c(q), {d: x.shape[1] for d, x in v.items()}, {d: x.shape[1] for d, x in k.items()},
                          heads, src, dst, V))
    return ref


def check_attention(name, mask, k, q, v, heads, out):
    B, L_ = mask.shape[:2]
    ref64, ref32 = attention_reference(mask, k, q, v, heads)
    for d in (0, 1):
        compare(f"{name} degree {d}", out[d], ref64[d], ref32[d])
    if L_ > 1:
        _, _, eid, _ = device_edges(mask, ceil64(int(mask.sum())))
        eid = eid.cpu()
        for b in range(B):
            for d in (0, 1):
                o = out[d].cpu()
                assert not o[b * L_ + 0].any()                                  # in-degree 0: exactly 0
                e = int(eid[b, L_ // 2, 1])                                     # in-degree 1: that edge's value
                torch.testing.assert_close(o[b * L_ + 1], v[d][e], rtol=4 * torch.finfo(F32).eps, atol=0)


@pytest.mark.parametrize("B,L_", [(1, 1), (1, 64), (1, 70), (2, 70), (1, 130)])
@pytest.mark.parametrize("cfg", HEADS, ids=[f"h{c[0]}-k{c[1]}_{c[2]}" for c in HEADS])
def test_se3_attention(B, L_, cfg):
    heads = cfg[0]
    mask = attention_mask(B, L_, seed=90 + L_)
    if L_ > 1:
        assert int(mask[0, :, 2].sum()) == L_ and int(mask[0, :, 1].sum()) == 1 and int(mask[0, :, 0].sum()) == 0
    k, q, v = attention_inputs(mask, *cfg, seed=91)
    out = run_attention(mask, k, q, v, heads)
    check_attention(f"se3_attention B={B} L={L_} heads={heads} mk=({cfg[1]},{cfg[2]})", mask, k, q, v, heads, out)
    if L_ == 1:   # the empty graph: the only node has no incoming edge
        z = run_attention(torch.zeros(B, 1, 1, dtype=torch.uint8), k, q, v, heads)
        assert not z[0].any() and not z[1].any()


@pytest.mark.parametrize("cfg", HEADS[:2], ids=["h4", "h1"])
@pytest.mark.parametrize("kind", ["large", "equal"])
def test_se3_attention_logits(cfg, kind):
    """logits of a few hundred (the softmax must subtract the maximum) and all-equal logits (the plain mean of the values)"""
    heads = cfg[0]
    mask = attention_mask(2, 70, seed=95)
    k, q, v = attention_inputs(mask, *cfg, seed=96, q_scale=(200.0 if heads == 4 else 100.0) if kind == "large" else 1.0,
                               equal=kind == "equal")
    src, dst = edge_list(mask)
    logit = sum((k[d].reshape(len(src), heads, -1) * q[d][dst].reshape(len(src), heads, -1)).sum(-1) for d in (0, 1))
    logit = logit / (cfg[1] + 3 * cfg[2]) ** 0.5
    if kind == "large":
        assert 200 < logit.abs().max() < 2000
    else:
        assert logit.abs().max() > 0.5 and torch.equal(logit[dst == 2], logit[dst == 2][:1].expand(70, heads))
    out = run_attention(mask, k, q, v, heads)
    check_attention(f"se3_attention {kind} logits heads={heads}", mask, k, q, v, heads, out)


@pytest.mark.parametrize("cfg", HEADS[:2], ids=["h4", "h1"])
def test_se3_attention_skip(cfg):
    """the GCat buffer: the attention writes the leading channels (bit for bit the run without skip), the skip tensors land
    behind them bit for bit"""
    heads, mv0, mv1 = cfg[0], cfg[3], cfg[4]
    mask = attention_mask(2, 70, seed=97)
    V = 140
    k, q, v = attention_inputs(mask, *cfg, seed=98)
    s0, s1 = randn(V, 8, 1, seed=99), randn(V, 3, 3, seed=100)
    plain = run_attention(mask, k, q, v, heads)
    both = run_attention(mask, k, q, v, heads, skip=(s0, s1))
    only0 = run_attention(mask, k, q, v, heads, skip=(s0, None))
    only1 = run_attention(mask, k, q, v, heads, skip=(None, s1))
    assert both[0].shape == (V, mv0 + 8, 1) and both[1].shape == (V, mv1 + 3, 3)
    assert only0[1].shape == plain[1].shape and only1[0].shape == plain[0].shape
    for got0, got1, has0, has1 in ((both[0], both[1], True, True), (only0[0], only0[1], True, False), (only1[0], only1[1], False, True)):
        assert torch.equal(got0[:, :mv0], plain[0]) and torch.equal(got1[:, :mv1], plain[1])
        if has0:
            assert torch.equal(got0[:, mv0:].cpu(), s0)
        if has1:
            assert torch.equal(got1[:, mv1:].cpu(), s1)
    check_attention(f"se3_attention skip heads={heads}", mask, k, q, v, heads, (both[0][:, :mv0], both[1][:, :mv1]))


# ------------------------------------------------------------------------------------------------ 6. small kernels
VS = 141   # V * m and V * m * m are no multiples of the 256-thread block


@pytest.mark.parametrize("deg", [0, 1])
def test_norm_bias(deg):
    m = 19
    v = randn(VS, m, 2 * deg + 1, seed=110 + deg)
    v[::5, 3] = 0.0                       # zero vectors: 0 out, no NaN
    bias = randn(m, seed=112)
    bias[7] = -50.0                       # more negative than every norm: exactly 0
    bias[3] = 0.5
    y = ops.se3_norm_bias(v.to(DEV), bias.to(DEV), deg).cpu()
    assert torch.isfinite(y).all() and not y[::5, 3].any() and not y[:, 7].any()
    ref = [O.gnorm_bias({"m.bias.%d" % deg: bias.view(1, m).to(dt)}, "m", {deg: v.to(dt)})[deg] for dt in (F64, F32)]
    compare(f"norm_bias degree {deg}", y, ref[0], ref[1])


def gram_reference(v):
    """the clamped-sign Gram matrix of oracle.gattentive_selfint"""
    s = torch.einsum("nac,nbc->nab", v, v).reshape(v.shape[0], -1)
    return s.abs().clamp_min(1e-12) * s.sign()


@pytest.mark.parametrize("deg", [0, 1])
def test_gram(deg):
    m = 19
    v = randn(VS, m, 2 * deg + 1, seed=120 + deg)
    if deg == 1:   # orthogonal integer vectors: their products are exactly 0
        v[:, 0] = torch.tensor([1.0, 2.0, 0.0])
        v[:, 1] = torch.tensor([2.0, -1.0, 0.0])
        v[:, 2] = torch.tensor([0.0, 0.0, 3.0])
    else:
        v[:, 0] = 0.0
    s = ops.se3_gram(v.to(DEV), deg).cpu()
    s3 = s.view(VS, m, m)
    if deg == 1:
        for a, b in ((0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)):
            assert not s3[:, a, b].any()
        assert torch.equal(s3[:, 0, 0], torch.full((VS,), 5.0))
    else:
        assert not s3[:, 0, :].any() and not s3[:, :, 0].any()
    compare(f"gram degree {deg}", s, gram_reference(v.double()), gram_reference(v))


@pytest.mark.parametrize("deg", [0, 1])
@pytest.mark.parametrize("m_in,m_out", [(19, 3), (19, 12), (32, 32), (32, 3)])
def test_attn_apply(m_in, m_out, deg):
    x = randn(VS, m_in, 2 * deg + 1, seed=130 + deg)
    scale = 10.0 ** (torch.rand(VS, 1, generator=gen(131)) * 3.0 - 1.0)       # per node 0.1 .. 100: flat to one-hot rows
    att = (randn(VS, m_out * m_in, seed=132) * scale).clamp(-200.0, 200.0)
    att[0, :m_in] = 200.0
    att[0, 1] = -200.0
    assert att.abs().max() == 200.0
    y = ops.se3_attn_apply(att.to(DEV), x.to(DEV), m_out, deg).cpu()
    ref = [torch.einsum("nom,nmd->nod", att.to(dt).view(VS, m_out, m_in).softmax(-1), x.to(dt)) for dt in (F64, F32)]
    compare(f"attn_apply m_in={m_in} m_out={m_out} degree {deg}", y, ref[0], ref[1])


def test_coord_apply_and_center_ca():
    """additions and subtractions only: exact"""
    B, L_ = 3, 47
    xyz, disp = chain(B, L_, seed=140), 0.3 * randn(B, L_, 3, 3, seed=141)
    ca = xyz[:, :, 1] + disp[:, :, 1]
    want = torch.stack([ca + disp[:, :, 0], ca, ca + disp[:, :, 2]], 2)
    assert torch.equal(ops.coord_apply(xyz.to(DEV), disp.to(DEV)).cpu(), want)
    assert torch.equal(ops.center_ca(xyz.to(DEV)).cpu(), xyz - xyz[:, :, 1].unsqueeze(-2))


# ------------------------------------------------------------------------------------------------ 7. the module, on the displacement
@pytest.mark.parametrize("k", [4, 32])
@pytest.mark.parametrize("d_state", [8, 16, 32, 12])
def test_coord_update_displacement(d_state, k, monkeypatch):
    """CoordUpdateWithMsaAndPair in the exact-fp32 mode against O.coord_update in float64, on `state` and on the displacement
    xyz_out - xyz_in (not on xyz_out: |xyz| is tens of angstroms, the displacement a fraction of one).  The kNN selection stays
    the oracle's own float32 rule on the float32 coordinates in both reference runs, so both sides build the same graph."""
    B, N, L_ = 2, 4, 70
    knn = O.knn_graph
    monkeypatch.setattr(O, "knn_graph", lambda xyz, idx, nn_, kmin=9: knn(xyz.float(), idx, nn_, kmin))
    m = build(lambda: R.CoordUpdateWithMsaAndPair(32, 24, 8, 8, d_state, n_neighbors=k, p_dropout=0.0), seed=150 + d_state)
    msa, pair, xyz = randn(B, N, L_, 32, seed=151), randn(B, L_, L_, 24, seed=152), chain(B, L_, seed=153)
    oh = torch.nn.functional.one_hot(torch.randint(0, 21, (B, L_), generator=gen(154)), 21).float()
    aa = torch.arange(L_).repeat(B, 1)
    aa[1, 40:] += 200
    R.set_compute_dtype(F32)
    try:
        st, xo = m(xyz.to(DEV), msa.to(DEV), pair.to(DEV), aa.to(DEV), oh.to(DEV))
    finally:
        R.set_compute_dtype(torch.bfloat16)
    ref = [O.coord_update(params(m, dt), "m", xyz.to(dt), msa.to(dt), pair.to(dt), aa, oh.to(dt), k, d_state) for dt in (F64, F32)]
    compare(f"coord_update d_state={d_state} k={k} state", st.reshape(B * L_, -1), ref[0][0].reshape(B * L_, -1),
            ref[1][0].reshape(B * L_, -1))
    disp = [(x.detach().cpu().double() - xyz.double()).reshape(B * L_, 9) for x in (xo, ref[0][1], ref[1][1])]
    assert 0.01 < disp[1].abs().max() < 0.2 * xyz.abs().max()
    compare(f"coord_update d_state={d_state} k={k} displacement", disp[0], disp[1], disp[2])
