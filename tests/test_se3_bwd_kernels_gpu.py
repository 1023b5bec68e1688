"""rf_se3_attention_bwd, rf_se3_norm_bias_bwd, rf_se3_gram_bwd, rf_se3_attn_apply_bwd and rf_layernorm_act_bwd (csrc/se3.hip):
the kernels the backward of GMABSE3, GNormBias and GAttentiveSelfInt adds, in both builds.

Each output is held against float64 autograd of the CPU oracle (oracle/rf_oracle.py: gmab, gnorm_bias, and the Gram / apply /
LayerNorm + LeakyReLU steps of gattentive_selfint restated one by one) on the same operands, by the yardstick rule of
tests/grad_oracle.py, with 2^-24, the rounding unit of the fp32 outputs.  Rows: one (node, head) of dq, one edge of dk / dv, one
(node, channel) vector of the node layers, one softmax row of datt, one LayerNorm row of dx, one element of a parameter
gradient.  The graphs come from hand-made masks through ops.edges_from_mask (the helper lines of tests/test_se3_kernels_gpu.py);
only the first n edge rows are compared, and the rows behind them must keep their sentinel.  Two runs must give the same bits.

RF_SE3_BACKWARD_ERRORS=FILE: the measured errors are also merged into that JSON file (key "kernel_errors")."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import grad_oracle as G  # noqa: E402
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import _lib, ops  # noqa: E402
from oracle import rf_oracle as O  # noqa: E402

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
BUILDS = [("bf16-build", torch.bfloat16), ("f16-build", torch.float16)]
SENTINEL = 7.0
EINVAL = -1     # RF_EINVAL (include/rfmi.h)
RECORDS = []
HELD = dict(units=G.UNIT[F32], rows=1, records=RECORDS, key="out")
_restore_mode = G.restore_mode()
_write_records = G.records_fixture("RF_SE3_BACKWARD_ERRORS", RECORDS, "max(torch float32 autograd vs float64, 2^-24)")

# graph attention: (B, L) of the mask -- one node with a self loop; two samples of 70 (node 0 at in-degree 0, node 1 at in-degree
# 1, node 2 at in-degree L); 130: three candidates per lane
MASKS = [(1, 1), (2, 70), (1, 130)]
HEADS = [(4, 4, 4, 4, 4), (1, 16, 3, 16, 3), (1, 32, 3, 32, 3)]   # (heads, mk0, mk1, mv0, mv1)
HEAD_IDS = [f"h{c[0]}-k{c[1]}_{c[2]}" for c in HEADS]
VS = 141                                    # V * m is no multiple of the 256-thread block
FIBERS = [(19, 3), (48, 32), (24, 8)]       # (m_in, m_out)
LN_WIDTHS = [1, 361, 576, 2304]             # 361 = 19^2 is no multiple of 4; 2304 = 48^2: nine strides of a 256-thread block
ZERO_NODE, ZERO_CH = 7, 4                   # the all-zero vector v[ZERO_NODE, ZERO_CH]


@pytest.fixture(params=BUILDS, ids=[b[0] for b in BUILDS])
def build(request):
    """the kernels take fp32 operands and are built into both libraries"""
    R.set_compute_dtype(request.param[1])
    return request.param[0]


def randn(*s, seed):
    return torch.randn(*s, generator=G.gen(seed))


def autograd(fn, inputs, weights, dtype):
    """d sum_i(fn(*inputs)[i] * weights[i]) / d inputs by torch on the CPU in `dtype`"""
    xs = [x.detach().cpu().to(dtype).requires_grad_() for x in inputs]
    out = fn(*xs)
    out = out if isinstance(out, (tuple, list)) else (out,)
    sum((o * w.detach().cpu().to(dtype)).sum() for o, w in zip(out, weights)).backward()
    return [x.grad if x.grad is not None else torch.zeros_like(x) for x in xs]


# ================================================================================================ rf_se3_attention_bwd
def ceil64(n):
    return max(64, (n + 63) // 64 * 64)


def attention_mask(B, L_, seed, empty=False):
    """p = 0.3; node 0 has no incoming edge, node 1 exactly one, node 2 one from every node (itself included)"""
    if L_ == 1:
        return torch.zeros(B, 1, 1, dtype=torch.uint8) if empty else torch.ones(B, 1, 1, dtype=torch.uint8)
    mask = (torch.rand(B, L_, L_, generator=G.gen(seed)) < 0.3).to(torch.uint8)
    mask[:, :, 0] = 0
    mask[:, :, 1] = 0
    mask[:, L_ // 2, 1] = 1
    mask[:, :, 2] = 1
    return mask


def edge_list(mask):
    b, i, j = torch.where(mask.bool())
    L_ = mask.shape[1]
    return b * L_ + i, b * L_ + j


@functools.lru_cache(maxsize=None)
def attention_case(B, L_, cfg, q_scale=1.0, empty=False):
    """mask, the device edge map and the operands (k, v per edge padded to the capacity; q, g per node), shared and left unchanged"""
    heads, mk0, mk1, mv0, mv1 = cfg
    mask = attention_mask(B, L_, seed=90 + L_, empty=empty)
    if L_ > 1:
        assert int(mask[0, :, 2].sum()) == L_ and int(mask[0, :, 1].sum()) == 1 and int(mask[0, :, 0].sum()) == 0
    n, V = int(mask.sum()), B * L_
    cap = ceil64(n)
    src, dst, eid, count = ops.edges_from_mask(mask.to(DEV).contiguous(), cap, zero_tail=True)
    assert count.tolist() == [n, n]
    seed = 9100 + 7 * L_ + mk0

    def edges(m, nc, sd):   # [cap, m, nc]: n drawn rows, zeros behind them
        t = torch.zeros(cap, m, nc)
        t[:n] = randn(n, m, nc, seed=sd)
        return t
    k0, k1 = edges(mk0, 1, seed), edges(mk1, 3, seed + 1)
    if q_scale != 1.0:   # large logits: every key is one common key plus 2 %, so a node's logits are hundreds with a spread of a few
        k0[:n], k1[:n] = k0[:1] + 0.02 * k0[:n], k1[:1] + 0.02 * k1[:n]
    c = dict(mask=mask, n=n, V=V, L=L_, cap=cap, eid=eid, cfg=cfg, k0=k0, k1=k1, v0=edges(mv0, 1, seed + 2), v1=edges(mv1, 3, seed + 3),
             q0=q_scale * randn(V, mk0, 1, seed=seed + 4), q1=q_scale * randn(V, mk1, 3, seed=seed + 5),
             g0=randn(V, mv0, 1, seed=seed + 6), g1=randn(V, mv1, 3, seed=seed + 7))
    c["dev"] = {key: c[key].to(DEV) for key in ("k0", "k1", "v0", "v1", "q0", "q1", "g0", "g1")}
    return c


def attention_autograd(c, dtype):
    heads, mk0, mk1, mv0, mv1 = c["cfg"]
    n, V = c["n"], c["V"]
    src, dst = edge_list(c["mask"])

    def fn(k0, k1, q0, q1, v0, v1):
        out = O.gmab({0: v0, 1: v1}, {0: k0, 1: k1}, {0: q0, 1: q1}, {0: mv0, 1: mv1}, {0: mk0, 1: mk1}, heads, src, dst, V)
        return out[0], out[1]
    ins = [c[key][:n] if key[0] in "kv" else c[key] for key in ("k0", "k1", "q0", "q1", "v0", "v1")]
    dk0, dk1, dq0, dq1, dv0, dv1 = autograd(fn, ins, (c["g0"], c["g1"]), dtype)
    return rows_of(c, dk0, dk1, dq0, dq1, dv0, dv1)


def rows_of(c, dk0, dk1, dq0, dq1, dv0, dv1):
    """the six gradients as three tensors of rows: dq [V, heads, .] (one (node, head)), dk and dv [n, .] (one edge)"""
    heads, n, V = c["cfg"][0], c["n"], c["V"]
    flat = lambda a, b: torch.cat([a[:n].reshape(n, -1), b[:n].reshape(n, -1)], -1)  # noqa: E731
    return {"dq": torch.cat([dq0.reshape(V, heads, -1), dq1.reshape(V, heads, -1)], -1), "dk": flat(dk0, dk1), "dv": flat(dv0, dv1)}


@functools.lru_cache(maxsize=None)
def attention_refs(B, L_, cfg, q_scale=1.0):
    c = attention_case(B, L_, cfg, q_scale)
    return attention_autograd(c, F64), attention_autograd(c, F32)


def run_attention_bwd(c, g0=None, g1=None):
    """the entry point on sentinel-filled outputs; the edge rows at and behind the edge count must keep the sentinel"""
    heads, mk0, mk1, mv0, mv1 = c["cfg"]
    d = c["dev"]
    g0, g1 = d["g0"] if g0 is None else g0, d["g1"] if g1 is None else g1
    outs = [torch.full_like(d[key], SENTINEL) for key in ("k0", "k1", "q0", "q1", "v0", "v1")]
    p_ = ops.ptr
    rc = _lib.lib.rf_se3_attention_bwd(p_(d["k0"]), p_(d["k1"]), p_(d["q0"]), p_(d["q1"]), p_(d["v0"]), p_(d["v1"]), p_(c["eid"]),
                                       p_(g0), p_(g1), g0.shape[1], 3 * g1.shape[1], *[p_(o) for o in outs], heads, mk0, mk1, mv0,
                                       mv1, c["V"], c["L"], ops.stream())
    assert rc == 0
    n = c["n"]
    for o in (outs[0], outs[1], outs[4], outs[5]):
        assert (o[n:] == SENTINEL).all() and not (o[:n] == SENTINEL).any()
    assert not (outs[2] == SENTINEL).any() and not (outs[3] == SENTINEL).any()      # every (node, head) slice of dq is written
    return outs


def check_exact_cases(c, outs):
    """in-degree 0: dq exactly 0; in-degree 1: dk exactly 0 on that edge, dq exactly 0, dv equal to g bit for bit"""
    dk0, dk1, dq0, dq1, dv0, dv1 = outs
    B, L_ = c["mask"].shape[:2]
    eid = c["eid"].cpu()
    for b in range(B):
        if L_ == 1:
            lone = [(b, int(eid[b, 0, 0]))]            # the self loop is the node's only edge
        else:
            assert not dq0[b * L_].any() and not dq1[b * L_].any()
            lone = [(b * L_ + 1, int(eid[b, L_ // 2, 1]))]
        for node, e in lone:
            assert e >= 0
            assert not dq0[node].any() and not dq1[node].any()
            assert not dk0[e].any() and not dk1[e].any()
            assert torch.equal(dv0[e], c["dev"]["g0"][node]) and torch.equal(dv1[e], c["dev"]["g1"][node])


@pytest.mark.parametrize("B,L_", MASKS)
@pytest.mark.parametrize("cfg", HEADS, ids=HEAD_IDS)
def test_attention_bwd_against_float64_autograd(B, L_, cfg, build):
    c = attention_case(B, L_, cfg)
    ref64, ref32 = attention_refs(B, L_, cfg)
    outs = run_attention_bwd(c)
    assert G.held(rows_of(c, *outs), ref64, ref32, f"{build} se3_attention_bwd B={B} L={L_} {cfg}", **HELD)
    check_exact_cases(c, outs)
    again = run_attention_bwd(c)                        # the same bits on a second run
    assert all(torch.equal(a, o) for a, o in zip(again, outs))


@pytest.mark.parametrize("cfg", HEADS, ids=HEAD_IDS)
def test_attention_bwd_of_the_empty_graph(cfg, build):
    """(B, L) = (1, 1) without its edge: no per-edge row is written, dq is exactly 0"""
    c = attention_case(1, 1, cfg, empty=True)
    assert c["n"] == 0
    outs = run_attention_bwd(c)
    assert not outs[2].any() and not outs[3].any()


@pytest.mark.parametrize("cfg", HEADS[:2], ids=HEAD_IDS[:2])
def test_attention_bwd_with_logits_of_a_few_hundred(cfg, build):
    """q scaled by 200 (four heads) / 100 (one head): the recomputed softmax must subtract the maximum.  The keys of a node differ
    by a few logit units only: with logits hundreds APART a softmax row is one-hot to within 1e-16, its gradient is the float64
    reference's own rounding noise, and no relative error of such a row means anything -- asserted on the CPU before the launch:
    even torch's float32 autograd resolves every row (error below 0.5), so the float64 reference has nine digits in each."""
    heads, mk0, mk1 = cfg[:3]
    q_scale = 200.0 if heads == 4 else 100.0
    c = attention_case(2, 70, cfg, q_scale)
    src, dst = edge_list(c["mask"])
    n = c["n"]
    logit = sum((c[k][:n].reshape(n, heads, -1) * c[q][dst].reshape(n, heads, -1)).sum(-1) for k, q in (("k0", "q0"), ("k1", "q1")))
    assert 200 < (logit / (mk0 + 3 * mk1) ** 0.5).abs().max() < 2000
    ref64, ref32 = attention_refs(2, 70, cfg, q_scale)
    assert all(G.errors(ref32[key], ref64[key])[1] < 0.5 for key in ref64)
    outs = run_attention_bwd(c)
    assert all(torch.isfinite(o).all() for o in outs)
    assert G.held(rows_of(c, *outs), ref64, ref32, f"{build} se3_attention_bwd large logits {cfg}", **HELD)
    check_exact_cases(c, outs)


@pytest.mark.parametrize("cfg", HEADS[:2], ids=HEAD_IDS[:2])
def test_attention_bwd_through_a_gcat_strided_gradient(cfg, build):
    """g as the leading channels of the concatenated buffer's gradient (8 and 3 skip channels behind them): the same bits as the
    packed call, through the ops wrapper"""
    mv0, mv1 = cfg[3], cfg[4]
    c = attention_case(2, 70, cfg)
    d = c["dev"]
    wide0 = torch.cat([d["g0"], randn(c["V"], 8, 1, seed=31).to(DEV)], 1).contiguous()
    wide1 = torch.cat([d["g1"], randn(c["V"], 3, 3, seed=32).to(DEV)], 1).contiguous()
    packed = run_attention_bwd(c)
    strided = run_attention_bwd(c, wide0, wide1)
    assert all(torch.equal(a, b) for a, b in zip(packed, strided))
    via_ops = ops.se3_attention_bwd(d["k0"], d["k1"], d["q0"], d["q1"], d["v0"], d["v1"], c["eid"], wide0, wide1, *cfg, c["V"], c["L"])
    n = c["n"]
    for i, (a, b) in enumerate(zip(via_ops, packed)):      # (dk0, dk1, dq0, dq1, dv0, dv1): the per-edge ones up to the edge count
        assert torch.equal(a, b) if i in (2, 3) else torch.equal(a[:n], b[:n])
    ref64, ref32 = attention_refs(2, 70, cfg)
    assert G.held(rows_of(c, *strided), ref64, ref32, f"{build} se3_attention_bwd GCat-strided g {cfg}", **HELD)


def test_attention_bwd_refusals():
    c = attention_case(2, 70, HEADS[0])
    d = c["dev"]
    args = (d["k0"], d["k1"], d["q0"], d["q1"], d["v0"], d["v1"], c["eid"], d["g0"], d["g1"])
    with pytest.raises(ValueError):
        ops.se3_attention_bwd(*args, *HEADS[0], 2 * 1025, 1025)                       # L > 1024
    with pytest.raises(ValueError):
        ops.se3_attention_bwd(*args, 3, 4, 4, 4, 4, c["V"], c["L"])                    # heads does not divide the channels
    with pytest.raises(ValueError):
        ops.se3_attention_bwd(*args[:7], d["g0"][:, :2].contiguous(), d["g1"], *HEADS[0], c["V"], c["L"])   # g narrower than mv0
    with pytest.raises(ValueError):
        ops.se3_attention_bwd(d["k0"].double(), *args[1:], *HEADS[0], c["V"], c["L"])
    p_ = ops.ptr
    outs = [torch.full_like(d[key], SENTINEL) for key in ("k0", "k1", "q0", "q1", "v0", "v1")]
    rc = _lib.lib.rf_se3_attention_bwd(*[p_(a) for a in args], 0, 0, *[p_(o) for o in outs], 4, 4, 4, 4, 4, 2 * 1025, 1025, ops.stream())
    assert rc == EINVAL
    rc = _lib.lib.rf_se3_attention_bwd(*[p_(a) for a in args[:8]], None, 0, 0, *[p_(o) for o in outs], 4, 4, 4, 4, 4, c["V"], c["L"],
                                       ops.stream())
    assert rc == EINVAL
    assert all((o == SENTINEL).all() for o in outs)     # refused before any launch


# ================================================================================================ the node layers
@functools.lru_cache(maxsize=None)
def fiber_input(m, deg):
    """v [VS, m, 2 deg + 1] with a few exact zeros and one all-zero vector, and a gradient of its shape"""
    v = randn(VS, m, 2 * deg + 1, seed=110 + deg + m)
    v.view(-1)[::37] = 0.0
    v[ZERO_NODE, ZERO_CH] = 0.0
    return v, randn(VS, m, 2 * deg + 1, seed=210 + deg + m)


# ---- rf_se3_norm_bias_bwd
@functools.lru_cache(maxsize=None)
def norm_bias_case(m, deg):
    """every third channel closed at every node (n + b <= 0), the others drawn around the norms' size: about a third of the
    (node, channel) pairs of those are closed too; the all-zero vector sits in an open channel"""
    v, g = fiber_input(m, deg)
    bias = randn(m, seed=310 + m) * 0.5 - (0.4 if deg == 0 else 1.2)
    bias[::3] = -50.0
    bias[ZERO_CH] = 0.5
    s = v.double().norm(dim=-1).clamp_min(1e-12) + bias.double()
    closed = (s <= 0).float().mean().item()
    assert 0.33 <= closed <= 0.67, closed
    assert (s <= 0)[:, ::3].all() and 0.1 < (s <= 0)[:, 1::3].float().mean() < 0.9
    assert s.abs().min() > 1e-6                         # no pair within rounding distance of relu's kink
    ref = [autograd(lambda v_, b_: O.gnorm_bias({"m.bias.%d" % deg: b_.view(1, m)}, "m", {deg: v_})[deg], (v, bias), (g,), dt)
           for dt in (F64, F32)]
    return v, g, bias, s <= 0, ref


@pytest.mark.parametrize("deg", [0, 1])
@pytest.mark.parametrize("m", [f[0] for f in FIBERS])
def test_norm_bias_bwd_against_float64_autograd(m, deg, build):
    v, g, bias, closed, ((dv64, db64), (dv32, db32)) = norm_bias_case(m, deg)
    dv, db = ops.se3_norm_bias_bwd(v.to(DEV), bias.to(DEV), g.to(DEV), deg)
    got = {"dv": dv, "dbias": db.view(m, 1)}
    assert G.held(got, {"dv": dv64, "dbias": db64.view(m, 1)}, {"dv": dv32, "dbias": db32.view(m, 1)},
                  f"{build} se3_norm_bias_bwd m={m} degree {deg}", **HELD)
    assert (dv.cpu()[closed] == 0).all() and (dv.cpu()[~closed] != 0).any(-1).all()     # relu's flat side: exact zeros
    assert (db.cpu()[::3] == 0).all()
    assert torch.isfinite(dv).all() and dv[ZERO_NODE, ZERO_CH].abs().max() > 1e9          # |v| = 0: t / 1e-12 times g
    dv2, db2 = ops.se3_norm_bias_bwd(v.to(DEV), bias.to(DEV), g.to(DEV), deg)
    assert torch.equal(dv2, dv) and torch.equal(db2, db)


# ---- rf_se3_gram_bwd
def gram(v):
    """the clamped-sign Gram matrix of O.gattentive_selfint"""
    s = torch.einsum("nac,nbc->nab", v, v).reshape(v.shape[0], -1)
    return s.abs().clamp_min(1e-12) * s.sign()


@functools.lru_cache(maxsize=None)
def gram_case(m, deg):
    v, _ = fiber_input(m, deg)
    ds = randn(VS, m * m, seed=410 + m + deg)
    return v, ds, [autograd(gram, (v,), (ds,), dt)[0] for dt in (F64, F32)]


@pytest.mark.parametrize("deg", [0, 1])
@pytest.mark.parametrize("m", [f[0] for f in FIBERS])
def test_gram_bwd_against_float64_autograd(m, deg, build):
    v, ds, (r64, r32) = gram_case(m, deg)
    dv = ops.se3_gram_bwd(v.to(DEV), ds.to(DEV), deg)
    assert G.held({"dv": dv}, {"dv": r64}, {"dv": r32}, f"{build} se3_gram_bwd m={m} degree {deg}", **HELD)
    assert not dv[ZERO_NODE, ZERO_CH].any()             # the all-zero vector: every product under the clamp
    assert torch.equal(ops.se3_gram_bwd(v.to(DEV), ds.to(DEV), deg), dv)
    base = randn(VS, m, 2 * deg + 1, seed=411)          # accumulation into the apply path's gradient: one fp64 add, one rounding
    acc = ops.se3_gram_bwd(v.to(DEV), ds.to(DEV), deg, dv=base.to(DEV))
    assert G.held({"dv+": acc}, {"dv+": r64 + base.double()}, {"dv+": r32 + base}, f"{build} se3_gram_bwd accumulate m={m} degree {deg}",
                  **HELD)


# ---- rf_se3_attn_apply_bwd
def apply(att, x, m_out):
    return torch.einsum("nom,nmd->nod", att.view(x.shape[0], m_out, x.shape[1]).softmax(-1), x)


@functools.lru_cache(maxsize=None)
def apply_case(m_in, m_out, deg):
    x, _ = fiber_input(m_in, deg)
    # logits at a level of +-150 per node with a spread of 0.1 .. 3 units: flat to peaked rows whose gradient float32 autograd still
    # resolves (asserted below; a row that is one-hot to within 1e-16 has a gradient of rounding noise in float64 too)
    scale = 10.0 ** (torch.rand(VS, 1, generator=G.gen(131)) * 1.5 - 1.0)
    att = randn(VS, m_out * m_in, seed=510 + m_in) * scale + 150.0 * randn(VS, 1, seed=509)
    g = randn(VS, m_out, 2 * deg + 1, seed=511 + m_in + deg)
    return att, x, g, [autograd(lambda a_, x_: apply(a_, x_, m_out), (att, x), (g,), dt) for dt in (F64, F32)]


@pytest.mark.parametrize("deg", [0, 1])
@pytest.mark.parametrize("m_in,m_out", FIBERS)
def test_attn_apply_bwd_against_float64_autograd(m_in, m_out, deg, build):
    att, x, g, ((da64, dx64), (da32, dx32)) = apply_case(m_in, m_out, deg)
    assert att.abs().max() > 200 and G.errors(da32.view(VS, m_out, m_in), da64.view(VS, m_out, m_in))[1] < 0.5
    datt, dx = ops.se3_attn_apply_bwd(att.to(DEV), x.to(DEV), g.to(DEV), m_out, deg)
    rows = lambda t: t.reshape(VS, m_out, m_in)  # noqa: E731  (one softmax row)
    assert G.held({"datt": rows(datt), "dx": dx}, {"datt": rows(da64), "dx": dx64}, {"datt": rows(da32), "dx": dx32},
                  f"{build} se3_attn_apply_bwd m_in={m_in} m_out={m_out} degree {deg}", **HELD)
    datt2, dx2 = ops.se3_attn_apply_bwd(att.to(DEV), x.to(DEV), g.to(DEV), m_out, deg)
    assert torch.equal(datt2, datt) and torch.equal(dx2, dx)


# ---- rf_layernorm_act_bwd
EPS = 1e-5


@functools.lru_cache(maxsize=None)
def layernorm_case(D, leaky):
    x = randn(VS, D, seed=610 + D) * 2.0 + 0.5
    g = randn(VS, D, seed=611 + D)
    gamma, beta = 1.0 + 0.3 * randn(D, seed=612 + D), 0.3 * randn(D, seed=613 + D)

    def fn(x_, ga_, be_):
        y = F.layer_norm(x_, (D,), ga_, be_, EPS)
        return F.leaky_relu(y, 0.01) if leaky else y
    return x, g, gamma, beta, [autograd(fn, (x, gamma, beta), (g,), dt) for dt in (F64, F32)]


@pytest.mark.parametrize("leaky", [True, False], ids=["leaky", "plain"])
@pytest.mark.parametrize("D", LN_WIDTHS)
def test_layernorm_act_bwd_against_float64_autograd(D, leaky, build):
    x, g, gamma, beta, (r64, r32) = layernorm_case(D, leaky)
    act = _lib.ACT_LEAKY if leaky else _lib.ACT_NONE
    run = lambda: ops.layernorm_act_bwd(x.to(DEV), g.to(DEV), gamma.to(DEV), beta.to(DEV), eps=EPS, act=act)  # noqa: E731
    dx, dgamma, dbeta = run()
    name = lambda r: {"dx": r[0], "dgamma": r[1].view(D, 1), "dbeta": r[2].view(D, 1)}  # noqa: E731
    got, ref64, ref32 = name((dx, dgamma, dbeta)), name(r64), name(r32)
    if D == 1:
        # a row of one value: xhat = 0 exactly, so dx and dgamma are exact zeros; torch's autograd returns rounding noise around
        # zero for both in either precision, which is no yardstick: they are checked as exact zeros and left out of the rule
        assert not dx.any() and not dgamma.any()
        got, ref64, ref32 = ({"dbeta": t["dbeta"]} for t in (got, ref64, ref32))
    assert G.held(got, ref64, ref32, f"{build} layernorm_act_bwd D={D} {'leaky' if leaky else 'plain'}", **HELD)
    assert all(torch.equal(a, b) for a, b in zip(run(), (dx, dgamma, dbeta)))


def test_node_layer_refusals():
    v, g = (t.to(DEV) for t in fiber_input(19, 1))
    bias = torch.zeros(19, device=DEV)
    with pytest.raises(ValueError):
        ops.se3_norm_bias_bwd(v, bias[:18].contiguous(), g, 1)
    with pytest.raises(ValueError):
        ops.se3_norm_bias_bwd(v, bias, g.transpose(0, 1), 1)
    with pytest.raises(ValueError):
        ops.se3_gram_bwd(v, torch.zeros(VS, 19 * 18, device=DEV), 1)
    with pytest.raises(ValueError):
        ops.se3_attn_apply_bwd(torch.zeros(VS, 3 * 19, device=DEV), v, g[:, :2].contiguous(), 3, 1)
    with pytest.raises(ValueError):
        ops.layernorm_act_bwd(v, g, torch.ones(3, device=DEV), torch.zeros(3, device=DEV), act=_lib.ACT_RELU)
    with pytest.raises(ValueError):
        ops.layernorm_act_bwd(v, g.double(), torch.ones(3, device=DEV), torch.zeros(3, device=DEV))
    p_ = ops.ptr
    dv, db = torch.full_like(v, SENTINEL), torch.full_like(bias, SENTINEL)
    assert _lib.lib.rf_se3_norm_bias_bwd(p_(v), p_(bias), p_(g), p_(dv), p_(db), VS, 19, 1, None, 0, ops.stream()) == EINVAL
    assert _lib.lib.rf_layernorm_act_bwd(p_(v), p_(g), p_(bias), p_(bias), EPS, _lib.ACT_LEAKY, p_(dv), None, None, VS * 19, 3, None, 0,
                                         ops.stream()) == EINVAL
    assert (dv == SENTINEL).all() and (db == SENTINEL).all()
