"""edge_mask in GraphTransformer / GraphTransformerBlock (rf.py:632-655) and the degree-proportional kernel behind it
(csrc/ops.hip: graph_attention_masked_kernel, rf_graph_attention_masked).

The rule: a row attends to its edges only (masked columns get probability exactly 0 and k, v, e there are not read); a row with
no edge attends uniformly, 1/L, to every column -- the reference's float32 result whenever the scaled logits lie in (-32, 32).

Kernel accuracy is held against a float64 restatement on the same rounded operands.  Its ceiling is 4 x the error of the
existing dense kernel against the unmasked float64 restatement on the same tensors, measured at run time, for the relative L2
error of the whole output and for the worst row (margin 4: a row of one or two edges averages no rounding error away).  The dense
figure is taken on the tensors before the masked positions are scaled by 100: scaled, every dense softmax would collapse onto one
column and measure no accumulation error at all."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import _lib, custom_ops, ops  # noqa: E402

DEV = "cuda"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SHAPES = [(2, 5, 4, 8), (1, 64, 3, 16), (2, 65, 4, 64), (1, 130, 1, 32), (1, 257, 4, 8)]
# (id, library's 16-bit type, operand dtype): fp32 operands, and the 16-bit type of each build
OPERANDS = [("fp32", torch.bfloat16, torch.float32), ("bf16", torch.bfloat16, torch.bfloat16),
            ("fp16", torch.float16, torch.float16)]
MODES = [(torch.float32, 2e-4), (torch.bfloat16, 4e-2), (torch.float16, 6e-3)]  # tests/test_modules_gpu.py::MODES
MARGIN = 4.0


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    R.set_compute_dtype(torch.bfloat16)


@pytest.fixture(params=OPERANDS, ids=[o[0] for o in OPERANDS])
def operand(request):
    R.set_compute_dtype(request.param[1])
    return request.param


def run(q, k, v, e, mask, H, scale, dropout=None):
    B, L, HD = q.shape
    out = torch.empty(B, L, HD, device=DEV, dtype=torch.float32)
    ops.graph_attention(q, k, v, e, out, B, L, H, HD // H, scale, dropout=dropout, mask=mask)
    return out


def oracle(q, k, v, e, mask, H, scale, keep=None, p=0.0):
    """float64 on the CPU, on the operands as given.  -> (out [B, L, H*d], scaled logits [B, H, L, L] before masking)"""
    q, k, v, e = (t.detach().double().cpu() for t in (q, k, v, e))
    B, L, HD = q.shape
    d = HD // H
    qh, kh, vh, eh = q.view(B, L, H, d), k.view(B, L, H, d), v.view(B, L, H, d), e.view(B, L, L, H, d)
    logit = (torch.einsum("bihd,bjhd->bhij", qh, kh) + torch.einsum("bihd,bijhd->bhij", qh, eh)) * scale
    x = logit
    if mask is not None:
        on = (mask.cpu() != 0)[:, None]
        empty = ~on.any(-1, keepdim=True)
        x = torch.where(empty, torch.zeros_like(logit), logit.masked_fill(~on, float("-inf")))
    att = x.softmax(-1)
    if keep is not None:
        att = att * keep.double().cpu() / (1.0 - p)
    out = torch.einsum("bhij,bjhd->bihd", att, vh) + torch.einsum("bhij,bijhd->bihd", att, eh)
    return out.reshape(B, L, HD), logit


def errors(got, want):
    """(relative L2 error of the whole output, worst relative L2 error of one (b, i) row); every element counts"""
    g, w = got.detach().double().cpu(), want.double()
    assert g.shape == w.shape and torch.isfinite(g).all()
    rows = (g - w).norm(dim=-1) / w.norm(dim=-1).clamp_min(1e-300)
    return ((g - w).norm() / w.norm()).item(), rows.max().item()


def mixed_mask(B, L, seed):
    """uint8 [B, L, L]: rows of degree 0, 1, 2, 63, 64, 65 and L (those that fit) in turn, random columns: asymmetric, and
    another assignment for every batch item."""
    g = torch.Generator().manual_seed(seed)
    degs = sorted({x for x in (0, 1, 2, 63, 64, 65, L) if x <= L})
    m = torch.zeros(B, L, L, dtype=torch.uint8)
    for b in range(B):
        for i in range(L):
            m[b, i, torch.randperm(L, generator=g)[: degs[(i + 3 * b) % len(degs)]]] = 1
    return m


@functools.lru_cache(maxsize=None)
def case(shape, op_id):
    """One set of tensors and float64 references per (shape, operand type), shared by the tests below and left unchanged."""
    B, L, H, d = shape
    dt = {o[0]: o[2] for o in OPERANDS}[op_id]
    g = torch.Generator().manual_seed(1000 + L)
    q, k, v = (torch.randn(B, L, H * d, generator=g).to(dt).to(DEV) for _ in range(3))
    e = torch.randn(B, L, L, H * d, generator=g).to(dt).to(DEV)
    mask = mixed_mask(B, L, 7 + L)
    assert not torch.equal(mask, mask.transpose(1, 2)) and (B == 1 or not torch.equal(mask[0], mask[1]))
    scale = d ** -0.5
    ref_dense, logit = oracle(q, k, v, e, None, H, scale)
    # launch A: e at the masked positions of every row that has an edge is scaled by 100 (a row without one reads all of e)
    has_edge = mask.sum(-1, keepdim=True) > 0
    fa = torch.where((mask == 0) & has_edge, 100.0, 1.0)[..., None].to(dt).to(DEV)
    e_a = e * fa
    ref_a, _ = oracle(q, k, v, e_a, mask, H, scale)
    # launch B: no row is empty and the last column is nobody's edge, so k, v of that column and e of every masked position
    # must not matter at all
    mask_b = mask.clone()
    mask_b[:, :, L - 1] = 0
    mask_b[:, :, 0] |= (mask_b.sum(-1) == 0).to(torch.uint8)
    ref_b, _ = oracle(q, k, v, e, mask_b, H, scale)
    k_b, v_b = k.clone(), v.clone()
    k_b[:, L - 1] *= 100
    v_b[:, L - 1] *= 100
    e_b = e * torch.where(mask_b == 0, 100.0, 1.0)[..., None].to(dt).to(DEV)
    kept = logit[(mask != 0)[:, None].expand_as(logit)]
    return dict(q=q, k=k, v=v, e=e, mask=mask.to(DEV), scale=scale, ref_dense=ref_dense, e_a=e_a, ref_a=ref_a,
                mask_b=mask_b.to(DEV), k_b=k_b, v_b=v_b, e_b=e_b, ref_b=ref_b, max_kept_logit=kept.abs().max().item())


# ---- 1. an all-ones mask is the dense kernel, bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_all_ones_mask_equals_the_dense_kernel_bitwise(shape, operand):
    c = case(shape, operand[0])
    B, L, H, d = shape
    ones = torch.ones(B, L, L, device=DEV, dtype=torch.uint8)
    for drop in (None, (0.3, 5, 0)):
        dense = torch.empty(B, L, H * d, device=DEV)
        ops.graph_attention(c["q"], c["k"], c["v"], c["e"], dense, B, L, H, d, c["scale"], dropout=drop)
        assert torch.equal(run(c["q"], c["k"], c["v"], c["e"], ones, H, c["scale"], dropout=drop), dense), drop


# ---- 2. the kernel against the float64 restatement --------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_kernel_against_float64(shape, operand):
    c = case(shape, operand[0])
    B, L, H, d = shape
    q, k, v, e, mask, scale = c["q"], c["k"], c["v"], c["e"], c["mask"], c["scale"]
    assert c["max_kept_logit"] < 32.0
    dense = torch.empty(B, L, H * d, device=DEV)
    ops.graph_attention(q, k, v, e, dense, B, L, H, d, scale)
    d_all, d_row = errors(dense, c["ref_dense"])
    assert d_all > 0 and d_row > 0

    def within(got, want, tag):
        m_all, m_row = errors(got, want)
        print(f"{operand[0]} {shape} {tag}: rel-L2 {m_all:.3e} (dense {d_all:.3e}, ratio {m_all / d_all:.2f}), "
              f"worst row {m_row:.3e} (dense {d_row:.3e}, ratio {m_row / d_row:.2f})")
        return m_all <= MARGIN * d_all and m_row <= MARGIN * d_row

    out_a = run(q, k, v, c["e_a"], mask, H, scale)
    assert within(out_a, c["ref_a"], "masked, e x100 at masked positions")
    # masked k, v, e are not read: scaling them by 100 changes no bit
    out_b = run(q, k, v, e, c["mask_b"], H, scale)
    assert within(out_b, c["ref_b"], "masked, dead column")
    assert torch.equal(run(q, c["k_b"], c["v_b"], c["e_b"], c["mask_b"], H, scale), out_b)
    # the check has teeth: the mask's axes swapped, or one column of one degree-1 row moved, must fail it
    assert not within(run(q, k, v, c["e_a"], mask.transpose(1, 2).contiguous(), H, scale), c["ref_a"], "(swapped axes)")
    planted = mask.clone()
    b0, i0 = (mask.sum(-1) == 1).nonzero()[0].tolist()
    j0 = int(mask[b0, i0].argmax())
    planted[b0, i0, j0], planted[b0, i0, (j0 + 1) % L] = 0, 1
    assert not within(run(q, k, v, c["e_a"], planted, H, scale), c["ref_a"], "(planted column)")


# ---- 3. what counts as an edge ----------------------------------------------------------------------------------------------
def test_any_nonzero_byte_is_an_edge_and_mask_dtypes_agree():
    c = case(SHAPES[2], "bf16")
    q, k, v, e, mask, scale = c["q"], c["k"], c["v"], c["e"], c["mask"], c["scale"]
    assert torch.equal(run(q, k, v, e, mask, 4, scale), run(q, k, v, e, mask * 255, 4, scale))
    torch.manual_seed(4)
    blk = R.GraphTransformerBlock(8, 8, 8, 4, 0.0).to(DEV)
    g = torch.Generator().manual_seed(2)
    node, edge = torch.randn(2, 16, 8, generator=g).to(DEV), torch.randn(2, 16, 16, 8, generator=g).to(DEV)
    m = (torch.rand(2, 16, 16, generator=g) < 0.4)
    y = blk(node, edge, m.float().to(DEV))
    assert torch.equal(y, blk(node, edge, m.to(DEV)))          # bool
    assert torch.equal(y, blk(node, edge, m.to(torch.uint8)))  # uint8, on the host: moved to the device
    assert torch.equal(y, blk(node, edge, m.double().to(DEV)))


# ---- 4. dropout on the masked probabilities ----------------------------------------------------------------------------------
def test_dropout_under_a_mask():
    B, L, H, d, p, seed, off = 2, 70, 4, 8, 0.3, 5, 3
    g = torch.Generator().manual_seed(21)
    q, k, v = (torch.randn(B, L, H * d, generator=g).to(DEV) for _ in range(3))
    e = torch.randn(B, L, L, H * d, generator=g).to(DEV)
    mask = mixed_mask(B, L, 9)
    mask[:, ::2] = 0
    mask[:, ::2].scatter_(-1, torch.randint(0, L, (B, (L + 1) // 2, 1), generator=g), 1)   # every other row: degree 1
    mask = mask.to(DEV)
    scale = d ** -0.5
    out = run(q, k, v, e, mask, H, scale, dropout=(p, seed, off))
    assert torch.equal(out, run(q, k, v, e, mask, H, scale, dropout=(p, seed, off)))
    assert not torch.equal(out, run(q, k, v, e, mask, H, scale, dropout=(p, seed + 1, off)))
    # the keep/drop decision of element [b, h, i, j] is rf_dropout's over the [B, H, L, L] map (include/rfmi.h)
    keep = ops.dropout(torch.ones(B, H, L, L, device=DEV), p, seed, off, out=torch.empty(B, H, L, L, device=DEV)) != 0
    want, _ = oracle(q, k, v, e, mask, H, scale, keep=keep, p=p)
    dense = torch.empty(B, L, H * d, device=DEV)
    ops.graph_attention(q, k, v, e, dense, B, L, H, d, scale, dropout=(p, seed, off))
    d_all, d_row = errors(dense, oracle(q, k, v, e, None, H, scale, keep=keep, p=p)[0])
    m_all, m_row = errors(out, want)
    print(f"dropout: rel-L2 {m_all:.3e} (dense {d_all:.3e}), worst row {m_row:.3e} (dense {d_row:.3e})")
    assert m_all <= MARGIN * d_all and m_row <= MARGIN * d_row
    # a row of degree 1: each head's block is exactly 0 (dropped) or (v_j + e_ij) / (1 - p) (kept)
    deg1 = (mask.sum(-1) == 1).nonzero()
    col = mask[deg1[:, 0], deg1[:, 1]].argmax(-1)
    got = out[deg1[:, 0], deg1[:, 1]].view(-1, H, d)
    term = (v[deg1[:, 0], col] + e[deg1[:, 0], deg1[:, 1], col]).view(-1, H, d)
    kept = keep[deg1[:, 0], :, deg1[:, 1], col]                              # [rows, H]
    assert kept.any() and (~kept).any()
    assert (got[~kept] == 0).all()
    torch.testing.assert_close(got[kept], term[kept] * (1.0 / (1.0 - p)), rtol=1e-6, atol=0)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def test_entry_point_refuses_before_a_launch():
    B, L, H, d = 1, 8, 4, 8
    q = torch.zeros(B, L, H * d, device=DEV)
    e = torch.zeros(B, L, L, H * d, device=DEV)
    mask = torch.ones(B, L, L, device=DEV, dtype=torch.uint8)
    out = torch.zeros(B, L, H * d, device=DEV)
    p_ = ops.ptr

    def call(mask_ptr, L_, p):
        return _lib.lib.rf_graph_attention_masked(p_(q), p_(q), p_(q), p_(e), _lib.RF_F32, mask_ptr, p_(out), B, L_, H, d, 0.3, p,
                                                  0, 0, ops.stream())

    assert call(p_(mask), L, 0.0) == 0
    assert call(p_(mask), L, 0.5) == 0
    assert call(None, L, 0.0) == -1            # RF_EINVAL: NULL mask
    assert call(p_(mask), L, 1.0) == -1        # p outside [0, 1)
    assert call(p_(mask), L, -0.1) == -1
    assert call(p_(mask), 3300, 0.0) == -1     # (H*L + L + 8) * 4 bytes of LDS > 64 KB: refused, nothing is launched
    torch.cuda.synchronize()


@pytest.mark.parametrize("block", [False, True], ids=["GraphTransformer", "GraphTransformerBlock"])
def test_modules_refuse_another_mask_shape(block):
    m = (R.GraphTransformerBlock if block else R.GraphTransformer)(8, 8, 8, 4, 0.0).to(DEV)
    node, edge = torch.zeros(2, 6, 8, device=DEV), torch.zeros(2, 6, 6, 8, device=DEV)
    for shape in ((2, 6), (2, 6, 7)):
        with pytest.raises(ValueError):
            m(node, edge, torch.ones(*shape, device=DEV))


# ---- 6. the modules in all three compute modes --------------------------------------------------------------------------------
def restate(P, node, edge, mask, H, block):
    """GraphTransformer (block: GraphTransformerBlock) in float64 under the masking rule of this file's docstring."""
    P = {k: v.detach().double().cpu() for k, v in P.items()}
    pre = "attn." if block else ""
    node, edge = node.double().cpu(), edge.double().cpu()
    B, L, _ = node.shape

    def lin(x, name, bias=True):
        y = x @ P[name + ".weight"].T
        return y + P[name + ".bias"] if bias else y

    q, k, v = (lin(node, pre + "node_to_" + c).view(B, L, H, -1) for c in "qkv")
    d = q.shape[-1]
    e = lin(edge, pre + "edge_emb", bias=False).view(B, L, L, H, d)
    logit = (torch.einsum("bihd,bjhd->bhij", q, k) + torch.einsum("bihd,bijhd->bhij", q, e)) * d ** -0.5
    if mask is not None:
        on = (mask.cpu() == 1)[:, None]
        empty = ~on.any(-1, keepdim=True)
        logit = torch.where(empty, torch.zeros_like(logit), logit.masked_fill(~on, float("-inf")))
    att = logit.softmax(-1)
    upd = torch.einsum("bhij,bjhd->bihd", att, v) + torch.einsum("bhij,bijhd->bihd", att, e)
    x = lin(node, pre + "node_update") + upd.reshape(B, L, H * d)
    if not block:
        return x
    x = torch.nn.functional.layer_norm(x, (H * d,), P["ln.weight"], P["ln.bias"], 1e-5)
    return torch.nn.functional.elu(lin(x, "to_out.0")) + node


def rel(a, b):
    """max |a-b| / max |b| (tests/test_modules_gpu.py)"""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-20)).item()


@pytest.mark.parametrize("mode", MODES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("block", [False, True], ids=["GraphTransformer", "GraphTransformerBlock"])
def test_modules_against_float64(block, mode):
    R.set_compute_dtype(mode[0])
    B, L, dn, H = 2, 16, 8, 4
    torch.manual_seed(11)
    m = (R.GraphTransformerBlock if block else R.GraphTransformer)(dn, dn, dn, H, 0.0).to(DEV)
    g = torch.Generator().manual_seed(6)
    node, edge = torch.randn(B, L, dn, generator=g), torch.randn(B, L, L, dn, generator=g)
    mask = (torch.rand(B, L, L, generator=g) < 0.4).float()
    mask[0, 3], mask[1, 0], mask[1, 5] = 0.0, 1.0, 0.0
    mask[1, 5, 7] = 1.0
    y = m(node.to(DEV), edge.to(DEV), mask.to(DEV))
    y0 = m(node.to(DEV), edge.to(DEV), None)
    assert not torch.equal(y, y0) and (y - y0).abs().max().item() > 0.1     # the mask is honoured, not dropped
    P = dict(m.state_dict())
    assert rel(y, restate(P, node, edge, mask, H, block)) < mode[1]
    assert rel(y0, restate(P, node, edge, None, H, block)) < mode[1]


def test_reference_fixture_through_the_module():
    z = np.load(os.path.join(GOLD, "graph_transformer_block_masked.npz"), allow_pickle=False)
    P = {k[2:]: torch.from_numpy(z[k]).float() for k in z.files if k.startswith("w:")}
    R.set_compute_dtype(torch.float32)
    m = R.GraphTransformerBlock(8, 8, 8, 4, 0.0)
    m.load_state_dict(P, strict=True)
    m = m.to(DEV)
    node, edge, mask = (torch.from_numpy(z["in:" + k]).to(DEV) for k in ("node", "edge", "edge_mask"))
    torch.testing.assert_close(m(node, edge, mask).cpu(), torch.from_numpy(z["out:y"]), rtol=1e-4, atol=2e-5)


# ---- 7. composition with the project's own mask builder, and the dispatcher op ----------------------------------------------
def test_knn_mask_through_the_custom_op():
    B, L, H, d = 2, 24, 4, 8
    g = torch.Generator().manual_seed(3)
    steps = torch.randn(B, L, 3, generator=g)
    ca = torch.cumsum(3.8 * steps / steps.norm(dim=-1, keepdim=True), 1)
    xyz = ca[:, :, None, :] + 0.5 * torch.randn(B, L, 3, 3, generator=g)
    xyz[:, :, 1] = ca
    aa_idx = torch.arange(L).repeat(B, 1)
    mask = ops.knn_mask(xyz.to(DEV), aa_idx.to(DEV), 4)
    assert mask.dtype == torch.uint8 and 0 < int(mask.sum()) < B * L * L
    q, k, v = (torch.randn(B, L, H, d, generator=g).to(ops.h16()).to(DEV) for _ in range(3))
    e = torch.randn(B, L, L, H * d, generator=g).to(ops.h16()).to(DEV)
    assert "graph_transformer_masked" in custom_ops.MASKED_OPS
    got = torch.ops.rfmi.graph_transformer_masked(q, k, v, e, mask, 0.35)
    want = run(q.view(B, L, H * d), k.view(B, L, H * d), v.view(B, L, H * d), e, mask, H, 0.35)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    torch.library.opcheck(torch.ops.rfmi.graph_transformer_masked.default, (q, k, v, e, mask, 0.35),
                          test_utils=("test_schema", "test_faketensor"))


# ---- 8. no host read-back: a masked call can be captured ---------------------------------------------------------------------
def test_masked_block_replays_from_a_captured_graph():
    torch.manual_seed(8)
    blk = R.GraphTransformerBlock(8, 8, 8, 4, 0.0).to(DEV)
    g = torch.Generator().manual_seed(12)
    node, edge = torch.randn(2, 16, 8, generator=g).to(DEV), torch.randn(2, 16, 16, 8, generator=g).to(DEV)
    mask = (torch.rand(2, 16, 16, generator=g) < 0.3).float().to(DEV)
    mask[0, 2] = 0.0
    eager = blk(node, edge, mask).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        blk(node, edge, mask)                  # weight copies are prepared outside the capture
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            out = blk(node, edge, mask)
    torch.cuda.current_stream().wait_stream(side)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
