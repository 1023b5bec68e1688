"""Backward pass of GraphTransformer / GraphTransformerBlock (enable_backward; rf.py:613-676) and the kernel behind it
(csrc/backward.hip: rf_graph_attention_bwd, rf_elu_bwd).

Kernel accuracy is held against float64 autograd of a restatement of the forward (the one of tests/test_edge_mask_gpu.py, made
differentiable) on the operands as rounded, by the yardstick rule of tests/grad_oracle.py.  The units are 2^-24 for the fp32 dq,
dk, dv and the operand type's unit for de.  A row is one (b, i); the margin is 4 because a row of one or two edges averages no
rounding error away.  A row whose float64 gradient is exactly zero (dq of a node with no or one edge) must be exactly zero.

The modules are held by the ceiling-or-kink-floor rule of the same file.  b_k moves every logit of a row by the same q_i . b_k,
which a softmax ignores (sum_j ds_ij = 0, under a mask and under dropout too): the exact gradient of node_to_k.bias is 0 and the
float64 reference holds only its own rounding noise, so a relative error has no denominator.  The gradient is sum_j dk_j, the sum
of the rows whose outer products with node_j make up node_to_k.weight's gradient: its error is taken against that gradient's norm
per input channel, under the same ceiling.

RF_GRAPH_BACKWARD_ERRORS=FILE: the measured kernel errors are also merged into that JSON file (key "kernel_errors")."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import grad_oracle as G  # noqa: E402
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import _lib, ops  # noqa: E402
from rosettafold_pytorch_amd.runtime import RT  # noqa: E402
from oracle import rf_oracle as O  # noqa: E402

DEV = "cuda"
SHAPES = [(2, 5, 4, 8), (1, 64, 3, 16), (2, 65, 4, 64), (1, 130, 1, 32), (1, 257, 4, 8)]
# (id, library's 16-bit type, operand dtype): fp32 operands, and the 16-bit type of each build
OPERANDS = [("fp32", torch.bfloat16, torch.float32), ("bf16", torch.bfloat16, torch.bfloat16),
            ("fp16", torch.float16, torch.float16)]
OP_DTYPE = {o[0]: o[2] for o in OPERANDS}
MASKS = ["none", "ones", "mixed"]
UNIT, CEIL, MODES = G.UNIT, G.CEIL, G.MODES
TINY = {torch.float16: 2.0 ** -25}   # half the spacing of fp16 below 2^-14: the rounding of a stored value that small
NAMES = ("dq", "dk", "dv", "de")
RECORDS = []
# de's storage type -> the units of the four gradients; a row is one (b, i): the last dimension of dq, dk, dv, the last two of de
UNITS = {dt: dict(dict.fromkeys(NAMES, G.UNIT[torch.float32]), de=G.UNIT[dt]) for dt in G.UNIT}
HELD = dict(rows={"dq": 1, "dk": 1, "dv": 1, "de": 2}, records=RECORDS)
CENTRED = lambda name: name.endswith("ln.weight")   # noqa: E731  the 1-D parameters drawn around 1
_restore_mode = G.restore_mode()
_write_records = G.records_fixture("RF_GRAPH_BACKWARD_ERRORS", RECORDS,
                                   "max(torch float32 autograd vs float64, unit of the storage type)")


@pytest.fixture(params=OPERANDS, ids=[o[0] for o in OPERANDS])
def operand(request):
    R.set_compute_dtype(request.param[1])
    return request.param


# ---- the forward, restated (any floating type, any device; differentiable) ---------------------------------------------------
def attention(q, k, v, e, mask, H, scale, keep=None, p=0.0):
    """q, k, v [B, L, H*d], e [B, L, L, H*d] -> out [B, L, H*d].  mask: None or [B, L, L] (nonzero = edge): a row attends to its
    edges only; a row with no edge attends uniformly with the constant logit 0.  keep [B, H, L, L]: the dropout's keep map."""
    B, L, HD = q.shape
    d = HD // H
    qh, kh, vh, eh = q.view(B, L, H, d), k.view(B, L, H, d), v.view(B, L, H, d), e.view(B, L, L, H, d)
    logit = (torch.einsum("bihd,bjhd->bhij", qh, kh) + torch.einsum("bihd,bijhd->bhij", qh, eh)) * scale
    if mask is not None:
        on = (mask.to(q.device) != 0)[:, None]
        empty = ~on.any(-1, keepdim=True)
        logit = torch.where(empty, torch.zeros_like(logit), logit.masked_fill(~on, float("-inf")))
    att = logit.softmax(-1)
    if keep is not None:
        att = att * (keep.to(att.dtype).to(q.device) / (1.0 - p))
    out = torch.einsum("bhij,bjhd->bihd", att, vh) + torch.einsum("bhij,bijhd->bihd", att, eh)
    return out.reshape(B, L, HD)


def autograd(q, k, v, e, g, mask, H, scale, dtype, keep=None, p=0.0, device="cpu"):
    """{dq, dk, dv, de} of sum(attention(...) * g) by torch autograd in `dtype` on the operands as given"""
    leaves = [t.detach().to(device).to(dtype).clone().requires_grad_() for t in (q, k, v, e)]
    (attention(*leaves, mask, H, scale, keep, p) * g.detach().to(device).to(dtype)).sum().backward()
    return {n: t.grad.detach().cpu() for n, t in zip(NAMES, leaves)}


def mixed_mask(B, L, seed):
    """uint8 [B, L, L]: rows of degree 0, 1, 2, 63, 64, 65 and L (those that fit) in turn, random columns: asymmetric, and
    another assignment for every batch item."""
    g = G.gen(seed)
    degs = sorted({x for x in (0, 1, 2, 63, 64, 65, L) if x <= L})
    m = torch.zeros(B, L, L, dtype=torch.uint8)
    for b in range(B):
        for i in range(L):
            m[b, i, torch.randperm(L, generator=g)[: degs[(i + 3 * b) % len(degs)]]] = 1
    return m


@functools.lru_cache(maxsize=None)
def case(shape, op_id):
    """One set of operands per (shape, operand type), shared by the tests below and left unchanged."""
    B, L, H, d = shape
    dt = OP_DTYPE[op_id]
    g_ = G.gen(2000 + L)
    q, k, v = (torch.randn(B, L, H * d, generator=g_).to(dt).to(DEV) for _ in range(3))
    e = torch.randn(B, L, L, H * d, generator=g_).to(dt).to(DEV)
    g = torch.randn(B, L, H * d, generator=g_).to(DEV)
    mask = mixed_mask(B, L, 11 + L)
    assert not torch.equal(mask, mask.transpose(1, 2)) and (B == 1 or not torch.equal(mask[0], mask[1]))
    return dict(q=q, k=k, v=v, e=e, g=g, scale=d ** -0.5, none=None, ones=torch.ones(B, L, L, dtype=torch.uint8).to(DEV),
                mixed=mask.to(DEV))


@functools.lru_cache(maxsize=None)
def refs(shape, op_id, mask_kind, drop=None):
    """(float64 autograd, float32 autograd) of the restatement on the case's operands; `ones` is `none`.  drop = (p, seed,
    offset): with the keep map rf_dropout draws over the [B, H, L, L] map."""
    if mask_kind == "ones":
        return refs(shape, op_id, "none", drop)
    c = case(shape, op_id)
    B, L, H, d = shape
    keep, p = None, 0.0
    if drop is not None:
        p = drop[0]
        keep = keep_map(B, H, L, drop).cpu()
    args = (c["q"], c["k"], c["v"], c["e"], c["g"], None if c[mask_kind] is None else c[mask_kind].cpu(), H, c["scale"])
    return autograd(*args, torch.float64, keep, p), autograd(*args, torch.float32, keep, p)


def keep_map(B, H, L, drop):
    p, seed, off = drop
    ones = torch.ones(B, H, L, L, device=DEV)
    return ops.dropout(ones, p, seed, off, out=torch.empty_like(ones)) != 0


def run_bwd(c, mask, H, dropout=None, **over):
    t = dict(c, **over)
    B, L, HD = t["q"].shape
    out = ops.graph_attention_bwd(t["q"], t["k"], t["v"], t["e"], t["g"], B, L, H, HD // H, t["scale"], dropout=dropout, mask=mask)
    return dict(zip(NAMES + ("pd", "ds"), out))


# ---- 1. the kernel against float64 autograd ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_kernel_against_float64_autograd(shape, operand, mask_kind):
    c = case(shape, operand[0])
    ref64, ref32 = refs(shape, operand[0], mask_kind)
    got = run_bwd(c, c[mask_kind], shape[2])
    assert got["dq"].dtype == got["dk"].dtype == got["dv"].dtype == torch.float32 and got["de"].dtype == operand[2]
    assert G.held(got, ref64, ref32, f"{operand[0]} {shape} mask={mask_kind}", UNITS[operand[2]], **HELD)
    if mask_kind == "mixed":   # the check has teeth: the mask's axes swapped must fail it
        swapped = run_bwd(c, c["mixed"].transpose(1, 2).contiguous(), shape[2])
        assert not G.held(swapped, ref64, ref32, f"{operand[0]} {shape} (swapped axes: must fail)", UNITS[operand[2]], **HELD)
        del RECORDS[-len(NAMES):]


def test_kernel_at_L_1024_H_4():
    """the longest row the issue names, in the 16-bit type: float64 and float32 autograd on the device"""
    R.set_compute_dtype(torch.bfloat16)
    B, L, H, d = 1, 1024, 4, 8
    g_ = G.gen(77)
    q, k, v = (torch.randn(B, L, H * d, generator=g_).to(torch.bfloat16).to(DEV) for _ in range(3))
    e = torch.randn(B, L, L, H * d, generator=g_).to(torch.bfloat16).to(DEV)
    g = torch.randn(B, L, H * d, generator=g_).to(DEV)
    c = dict(q=q, k=k, v=v, e=e, g=g, scale=d ** -0.5)
    got = run_bwd(c, None, H)
    args = (q, k, v, e, g, None, H, c["scale"])
    ref64 = autograd(*args, torch.float64, device=DEV)
    ref32 = autograd(*args, torch.float32, device=DEV)
    assert G.held(got, ref64, ref32, f"bf16 {(B, L, H, d)} mask=none", UNITS[torch.bfloat16], **HELD)


# ---- 2. exact facts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[4]], ids=str)
def test_exact_facts(shape, operand):
    c = case(shape, operand[0])
    B, L, H, d = shape
    mask, g = c["mixed"], c["g"]
    deg = mask.sum(-1)
    got = run_bwd(c, mask, H)
    # (a) de and both maps are exactly 0 at the masked columns of every row that has an edge
    dead = (mask == 0) & (deg > 0)[..., None]                      # [B, L, L]
    assert dead.any()
    assert (got["de"][dead] == 0).all()
    for m in ("pd", "ds"):
        assert got[m].shape == (B, H, L, L) and got[m].dtype == torch.float32
        assert (got[m][dead[:, None].expand(B, H, L, L)] == 0).all()
    # (b) an all-ones mask gives the dense call's bits, with and without dropout
    for drop in (None, (0.3, 5, 2)):
        dense, ones = run_bwd(c, None, H, dropout=drop), run_bwd(c, c["ones"], H, dropout=drop)
        for n in dense:
            assert torch.equal(dense[n], ones[n]), (n, drop)
    # (c) k, v at a column that is nobody's edge, and e at the masked positions of rows that have an edge, are never read
    mask_b = mask.clone()
    mask_b[:, :, L - 1] = 0
    mask_b[:, :, 0] |= (mask_b.sum(-1) == 0).to(torch.uint8)
    k_b, v_b = c["k"].clone(), c["v"].clone()
    k_b[:, L - 1] *= 100
    v_b[:, L - 1] *= 100
    e_b = c["e"] * torch.where(mask_b == 0, 100.0, 1.0)[..., None].to(c["e"].dtype)
    plain, scaled = run_bwd(c, mask_b, H), run_bwd(c, mask_b, H, k=k_b, v=v_b, e=e_b)
    for n in plain:
        assert torch.equal(plain[n], scaled[n]), n
    # (d) a row with no edge: dq exactly 0, ds exactly 0, de_ij = g_i / L within the rounding of the storage type
    eb, ei = (deg == 0).nonzero(as_tuple=True)
    assert len(eb) > 0
    assert (got["dq"][eb, ei] == 0).all() and (got["ds"][eb, :, ei] == 0).all()
    want = (g[eb, ei] / L)[:, None, :].expand(-1, L, -1)
    torch.testing.assert_close(got["de"][eb, ei].float(), want, rtol=4 * UNIT[operand[2]], atol=TINY.get(operand[2], 0.0))
    # (e) a row of one edge: ds = 0, so dq = 0
    ob, oi = (deg == 1).nonzero(as_tuple=True)
    assert len(ob) > 0
    assert (got["ds"][ob, :, oi] == 0).all() and (got["dq"][ob, oi] == 0).all()
    # (f) with dropout, a row of one edge: de at its edge is g_i / (1 - p) per head where the element was kept, exactly 0 where
    # it was dropped
    p, seed, off = 0.25, 9, 3
    keep = keep_map(B, H, L, (p, seed, off))
    dropped = run_bwd(c, mask, H, dropout=(p, seed, off))
    col = mask[ob, oi].argmax(-1)
    de1 = dropped["de"][ob, oi, col].float().view(-1, H, d)
    kept = keep[ob, :, oi, col]                                     # [rows, H]
    assert kept.any() and (~kept).any()
    assert (de1[~kept] == 0).all()
    torch.testing.assert_close(de1[kept], (g[ob, oi].view(-1, H, d) * (1.0 / (1.0 - p)))[kept], rtol=4 * UNIT[operand[2]], atol=TINY.get(operand[2], 0.0))


# ---- 3. dropout replay ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_kind", ["none", "mixed"])
def test_dropout_replay(operand, mask_kind):
    shape, drop = SHAPES[2], (0.25, 1234, 5)
    c = case(shape, operand[0])
    ref64, ref32 = refs(shape, operand[0], mask_kind, drop)
    got = run_bwd(c, c[mask_kind], shape[2], dropout=drop)
    assert G.held(got, ref64, ref32, f"{operand[0]} {shape} mask={mask_kind} dropout={drop[0]}", UNITS[operand[2]], **HELD)
    again = run_bwd(c, c[mask_kind], shape[2], dropout=drop)
    other = run_bwd(c, c[mask_kind], shape[2], dropout=(drop[0], drop[1] + 1, drop[2]))
    for n in NAMES:
        assert torch.equal(got[n], again[n]) and not torch.equal(got[n], other[n]), n
    plain64, _ = refs(shape, operand[0], mask_kind)     # and the dropout matters: the reference without it is far away
    assert G.rel(got["dq"], plain64["dq"]) > 0.1


# ---- rf_elu_bwd ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", MODES)
def test_elu_bwd_against_cpu(dtype):
    R.set_compute_dtype(dtype)
    g_ = G.gen(5)
    n = 4099
    x, z, gy = (torch.randn(n, generator=g_) for _ in range(3))
    y = x + torch.nn.functional.elu(z)
    da = ops.elu_bwd(gy.to(DEV), y.to(DEV), x.to(DEV), dtype)
    zd = z.double().requires_grad_()
    (torch.nn.functional.elu(zd) * gy.double()).sum().backward()
    # a = y - x carries the fp32 rounding of y: 2^-23 |y| against a derivative of order 1
    assert da.dtype == dtype and G.rel(da, zd.grad) < max(4 * UNIT[dtype], 1e-6)
    assert torch.equal(ops.elu_bwd(gy.to(DEV), torch.nn.functional.elu(z).to(DEV), None, dtype),
                       ops.elu_bwd(gy.to(DEV), torch.nn.functional.elu(z).to(DEV), torch.zeros(n, device=DEV), dtype))


# ---- 4. the modules through the public surface ---------------------------------------------------------------------------------
def restate(P, pre, node, edge, mask, H, block, keep=None, p=0.0):
    """GraphTransformer (block: GraphTransformerBlock) in node's floating type under the masking rule of `attention`."""
    a = pre + ".attn" if block else pre

    def lin(x, name):
        y = x @ P[name + ".weight"].T
        return y + P[name + ".bias"] if name + ".bias" in P else y

    B, L, _ = node.shape
    q, k, v = (lin(node, f"{a}.node_to_{c}") for c in "qkv")
    HD = q.shape[-1]
    upd = attention(q, k, v, lin(edge, a + ".edge_emb"), mask, H, (HD // H) ** -0.5, keep, p)
    x = lin(node, a + ".node_update") + upd
    if not block:
        return x
    x = torch.nn.functional.layer_norm(x, (HD,), P[pre + ".ln.weight"], P[pre + ".ln.bias"], 1e-5)
    return torch.nn.functional.elu(lin(x, pre + ".to_out.0")) + node


def check(got, ref, floor, dtype, tag):
    """G.compare with every node_to_k.bias taken against its weight's gradient norm per input channel (the docstring above)"""
    norms = {}
    for key in ref:
        if key.endswith("node_to_k.bias"):
            wref = ref[key[:-len("bias")] + "weight"]
            norms[key] = wref.norm().item() / wref.shape[1] ** 0.5
    G.compare(got, ref, dtype, tag, floor, norms=norms)


def make(block, dn, H, p_dropout=0.0, seed=0):
    torch.manual_seed(100 + seed + dn)
    cls = R.GraphTransformerBlock if block else R.GraphTransformer
    return G.randomize(cls(dn, dn, dn, H, p_dropout).to(DEV), 7 + seed, CENTRED)


def inputs(B, L, dn, dtype, seed):
    g_ = G.gen(seed)
    node = torch.randn(B, L, dn, generator=g_).to(dtype).float()
    edge = torch.randn(B, L, L, dn, generator=g_).to(dtype).float()
    return node, edge


@pytest.mark.parametrize("dtype", MODES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("masked", [False, True], ids=["dense", "mixed-mask"])
@pytest.mark.parametrize("L,dn", [(16, 8), (16, 32), (65, 8), (65, 32)])
@pytest.mark.parametrize("block", [False, True], ids=["GraphTransformer", "GraphTransformerBlock"])
def test_module_grads_against_float64(block, L, dn, masked, dtype):
    R.set_compute_dtype(dtype)
    B, H = 2, 4
    mod = make(block, dn, H).enable_backward()
    node, edge = inputs(B, L, dn, dtype, 31 + L)
    w = torch.randn(B, L, dn if block else H * dn, generator=G.gen(L + dn))
    mask = mixed_mask(B, L, 5 + L) if masked else None
    got, _ = G.grads_of(mod, {"node": node, "edge": edge, "mask": mask}, w)
    if masked:
        fn = lambda P, nd, ed: restate(P, "m", nd, ed, mask, H, block)  # noqa: E731
    else:
        fn = lambda P, nd, ed: (O.graph_transformer_block if block else O.graph_transformer)(P, "m", nd, ed, H)  # noqa: E731
    ref, floor = G.oracle_grads(fn, G.state(mod), {"node": node, "edge": edge}, w, UNIT[dtype])
    assert all(t is not None for t in got.values()), got
    check(got, ref, floor, dtype, f"{'block' if block else 'attn'} L={L} dn={dn} masked={masked}")
    # the set of gradients _backward returns is the set of parameters
    tape = {}
    y = mod.run(node.to(DEV), ops.cast(edge.to(DEV), dtype), None if mask is None else mask.to(DEV), tape=tape)
    grads = mod._backward(tape, torch.ones_like(y))[2]
    assert set(grads) == set(mod.parameters())


# ---- 5. training mode ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", MODES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("masked", [False, True], ids=["dense", "mixed-mask"])
@pytest.mark.parametrize("block", [False, True], ids=["GraphTransformer", "GraphTransformerBlock"])
def test_training_mode_replays_the_attention_dropout(block, masked, dtype):
    R.set_compute_dtype(dtype)
    B, L, dn, H, p, seed = 2, 16, 8, 4, 0.25, 77
    mod = make(block, dn, H, p_dropout=p, seed=1).enable_backward()
    node, edge = inputs(B, L, dn, dtype, 41)
    w = torch.randn(B, L, dn if block else H * dn, generator=G.gen(43))
    mask = mixed_mask(B, L, 17) if masked else None
    with torch.no_grad():
        plain = mod(node.to(DEV), edge.to(DEV), mask)
    mod.train()
    runs = []
    for _ in range(2):
        R.manual_seed(seed)
        got, out = G.grads_of(mod, {"node": node, "edge": edge, "mask": mask}, w)
        runs.append([out] + [t.clone() for t in got.values()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert not torch.equal(runs[0][0], plain)   # the dropout acts
    # the one dropout of the forward takes the counters from 0 on (R.manual_seed): its keep map, replayed in the reference
    keep = keep_map(B, H, L, (p, seed, 0)).cpu()
    assert RT.train_seed == seed and RT.train_offset == (B * H * L * L + 3) // 4
    fn = lambda P, nd, ed: restate(P, "m", nd, ed, mask, H, block, keep, p)  # noqa: E731
    ref, floor = G.oracle_grads(fn, G.state(mod), {"node": node, "edge": edge}, w, UNIT[dtype])
    check(got, ref, floor, dtype, f"{'block' if block else 'attn'} train masked={masked}")


# ---- 6. the forward is unchanged --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", MODES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("block", [False, True], ids=["GraphTransformer", "GraphTransformerBlock"])
def test_forward_bits_unchanged(block, dtype):
    R.set_compute_dtype(dtype)
    B, L, dn, H = 2, 65, 8, 4
    twin = make(block, dn, H)
    mod = copy.deepcopy(twin).enable_backward()
    assert not twin._rf_backward
    node, edge = inputs(B, L, dn, dtype, 51)
    node, edge = node.to(DEV), edge.to(DEV)
    for mask in (None, mixed_mask(B, L, 3).to(DEV)):
        with torch.no_grad():
            want = twin(node, edge, mask)
            assert torch.equal(mod(node, edge, mask), want)
        got = mod(node.clone().requires_grad_(), edge, mask)
        assert got.requires_grad and torch.equal(got.detach(), want)
        assert not twin(node.clone().requires_grad_(), edge, mask).requires_grad   # the twin never records


# ---- 7. fp16: a small loss does not underflow -------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [False, True], ids=["GraphTransformer", "GraphTransformerBlock"])
def test_fp16_small_loss_does_not_underflow(block):
    R.set_compute_dtype(torch.float16)
    B, L, dn, H = 2, 16, 8, 4
    mod = make(block, dn, H, seed=2).enable_backward()
    node, edge = inputs(B, L, dn, torch.float16, 61)
    w = torch.randn(B, L, dn if block else H * dn, generator=G.gen(63))
    mask = mixed_mask(B, L, 19)
    small = 2.0 ** -20
    got, _ = G.grads_of(mod, {"node": node, "edge": edge, "mask": mask}, w * small)
    fn = lambda P, nd, ed: restate(P, "m", nd, ed, mask, H, block)  # noqa: E731
    ref, floor = G.oracle_grads(fn, G.state(mod), {"node": node, "edge": edge}, w, UNIT[torch.float16])
    for key, t in got.items():
        assert torch.isfinite(t).all() and t.abs().max() > 0, key
    check({key: t / small for key, t in got.items()}, ref, floor, torch.float16, f"{'block' if block else 'attn'} small loss")


# ---- 8. determinism and refusals -----------------------------------------------------------------------------------------------
def test_backward_is_deterministic():
    R.set_compute_dtype(torch.bfloat16)
    B, L, dn, H = 2, 65, 32, 4
    mod = make(True, dn, H, seed=3).enable_backward()
    node, edge = inputs(B, L, dn, torch.bfloat16, 71)
    w = torch.randn(B, L, dn, generator=G.gen(73))
    runs = []
    for _ in range(2):
        got, _ = G.grads_of(mod, {"node": node, "edge": edge, "mask": mixed_mask(B, L, 23)}, w)
        runs.append([t.clone() for t in got.values()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    c = case(SHAPES[4], "bf16")
    a, b = run_bwd(c, c["mixed"], 4, dropout=(0.25, 3, 1)), run_bwd(c, c["mixed"], 4, dropout=(0.25, 3, 1))
    assert all(torch.equal(a[n], b[n]) for n in a)


def test_entry_point_refuses_before_a_launch():
    R.set_compute_dtype(torch.bfloat16)
    B, L, H, d = 1, 8, 4, 8
    q = torch.zeros(B, L, H * d, device=DEV)
    e = torch.zeros(B, L, L, H * d, device=DEV)
    outs = [torch.zeros(B, L, H * d, device=DEV) for _ in range(3)]
    de = torch.zeros(B, L, L, H * d, device=DEV)
    maps = [torch.zeros(B, H, L, L, device=DEV) for _ in range(2)]
    p_ = ops.ptr

    def call(L_=L, H_=H, d_=d, p=0.0, ld=None):
        return _lib.lib.rf_graph_attention_bwd(p_(q), p_(q), p_(q), p_(e), _lib.RF_F32, None, p_(q), p_(outs[0]), p_(outs[1]),
                                               p_(outs[2]), p_(de), p_(maps[0]), p_(maps[1]), L_ if ld is None else ld, B, L_, H_, d_,
                                               0.3, p, 0, 0, ops.stream())

    assert call() == 0
    assert call(p=0.5) == 0
    assert call(H_=5, d_=64) == -1      # RF_EINVAL: H*d > 256
    assert call(d_=12) == -1            # d not a power of two
    assert call(p=1.0) == -1            # p outside [0, 1)
    assert call(p=-0.1) == -1
    assert call(ld=L - 1) == -1         # map_ld < L
    assert call(L_=1587) == -1          # (2*H*L + 2*L + 520) * 4 bytes of LDS > 64 KB at H = 4: refused, nothing is launched
    torch.cuda.synchronize()


@pytest.mark.parametrize("block", [False, True], ids=["GraphTransformer", "GraphTransformerBlock"])
def test_channel_counts_must_be_multiples_of_8_when_recording(block):
    R.set_compute_dtype(torch.float32)
    cls = R.GraphTransformerBlock if block else R.GraphTransformer
    mod = cls(12, 4, 8, 3, 0.0).to(DEV)     # d_node_in 12, H * d = 12
    node, edge = torch.randn(1, 6, 12, device=DEV), torch.randn(1, 6, 6, 8, device=DEV)
    plain = mod(node.clone().requires_grad_(), edge, None)      # not opted in: nothing records, nothing to refuse
    mod.enable_backward()
    with torch.no_grad():
        assert torch.equal(mod(node, edge, None), plain)
    with pytest.raises(ValueError):
        mod(node.clone().requires_grad_(), edge, None)
