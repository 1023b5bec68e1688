"""Backward pass of GNormBias, G1x1SE3, GAttentiveSelfInt and GMABSE3 (enable_backward): every parameter gradient and the gradient
of every input degree against float64 autograd through the CPU oracle (oracle/rf_oracle.py: gnorm_bias, g1x1, gattentive_selfint,
gmab with the skip concatenation behind it), with loss = sum over the output degrees of sum(out * w) for random w.

The ceiling-or-kink-floor rule of tests/grad_oracle.py at the fp32 ceiling 1e-4 in EVERY compute mode: the structure track is fp32
whatever set_compute_dtype says, and the gradients under bfloat16 and float32 are the same bits.  relu(norm + b) and the
LeakyReLU are kinks, so the references come with their kink floors at the fp32 rounding unit.  Also: forward numbers under
recording are bit-identical to run() without a tape, a loss of 2^-20 in the fp16 mode gives 2^-20 times the gradient,
determinism, and the refusal of a chain beyond 1024 before any launch.

Shapes: V = 2 * 35 nodes; fibers {0: 16, 1: 16}, the final layer's {0: 48, 1: 19} -> {0: 32, 1: 3}, and the q form
{0: 16, 1: 3} -> {0: 4} of G1x1SE3, whose output has fewer degrees than its input; the attention on a hand-made (2, 35) mask
(node 0 at in-degree 0, node 1 at in-degree 1, node 2 at in-degree L), with and without skip.  Only the first n rows of the
per-edge gradients are compared: the rows behind the edge count are not written."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import grad_oracle as G  # noqa: E402
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import ops, structure as S  # noqa: E402
from oracle import rf_oracle as O  # noqa: E402

DEV = "cuda"
F32 = torch.float32
UNIT = G.UNIT[F32]
B, LR = 2, 35
V = B * LR
_restore_mode = G.restore_mode()

# name -> (constructor, input fiber, oracle forward on (P, h))
LAYERS = {
    "norm_bias": (lambda: S.GNormBias({0: 16, 1: 16}), {0: 16, 1: 16}, lambda P, h: O.gnorm_bias(P, "m", h)),
    "norm_bias_final": (lambda: S.GNormBias({0: 32, 1: 3}), {0: 32, 1: 3}, lambda P, h: O.gnorm_bias(P, "m", h)),
    "g1x1": (lambda: S.G1x1SE3({0: 16, 1: 16}, {0: 16, 1: 16}), {0: 16, 1: 16}, lambda P, h: O.g1x1(P, "m", h, [0, 1])),
    "g1x1_final": (lambda: S.G1x1SE3({0: 48, 1: 19}, {0: 32, 1: 3}), {0: 48, 1: 19}, lambda P, h: O.g1x1(P, "m", h, [0, 1])),
    "g1x1_q": (lambda: S.G1x1SE3({0: 16, 1: 3}, {0: 4}), {0: 16, 1: 3}, lambda P, h: O.g1x1(P, "m", h, [0])),
    "selfint": (lambda: S.GAttentiveSelfInt({0: 16, 1: 16}, {0: 16, 1: 16}), {0: 16, 1: 16},
                lambda P, h: O.gattentive_selfint(P, "m", h, {0: 16, 1: 16})),
    "selfint_final": (lambda: S.GAttentiveSelfInt({0: 48, 1: 19}, {0: 32, 1: 3}), {0: 48, 1: 19},
                      lambda P, h: O.gattentive_selfint(P, "m", h, {0: 32, 1: 3})),
}


def randn(*s, seed):
    return torch.randn(*s, generator=G.gen(seed))


def weighted(out, w):
    return sum((out[d] * w[d].to(out[d].device, out[d].dtype)).sum() for d in out)


# ================================================================================================ the node layers
@functools.lru_cache(maxsize=None)
def layer_setup(name):
    """module (fp32 weights, CPU; LayerNorm affines and biases off 1 / 0), input fiber and loss weights, shared and left unchanged"""
    ctor, fiber, fn = LAYERS[name]
    seed = 100 + sum(map(ord, name))
    torch.manual_seed(seed)
    mod = G.randomize(ctor(), seed + 1, lambda n: n.endswith("0.weight"))
    h = {d: randn(V, m, 2 * d + 1, seed=seed + 2 + d) for d, m in fiber.items()}
    with torch.no_grad():
        out = fn(G.state(mod), {d: x.double() for d, x in h.items()})
    w = {d: randn(*o.shape, seed=seed + 10 + d) for d, o in out.items()}
    return mod, h, w


@functools.lru_cache(maxsize=None)
def layer_reference(name):
    mod, h, w = layer_setup(name)
    fn = LAYERS[name][2]
    return G.oracle_grads(lambda P, h0, h1: fn(P, {0: h0, 1: h1}), G.state(mod), {"h0": h[0], "h1": h[1]},
                          lambda out: weighted(out, w), unit=UNIT, seed=7)


def layer_backward(mod, h, w, scale=1.0):
    """the dict-aware twin of G.grads_of: ({m.name: parameter gradient, h0 / h1: input gradient or None}, detached outputs)"""
    for p in mod.parameters():
        p.grad = None
    xs = {d: x.detach().to(DEV).requires_grad_() for d, x in h.items()}
    out = mod(xs)
    (weighted(out, w) * scale).backward()
    grads = {f"m.{n}": p.grad for n, p in mod.named_parameters()}
    grads.update({f"h{d}": x.grad for d, x in xs.items()})
    return grads, {d: o.detach() for d, o in out.items()}


@pytest.mark.parametrize("name", list(LAYERS))
def test_node_layer_grads_against_oracle(name):
    mod, h, w = layer_setup(name)
    ref, floor = layer_reference(name)
    with G.recording(mod):
        got, _ = layer_backward(mod, h, w)
    unread = [k for k in got if k not in ref]
    assert unread == (["h1"] if name == "g1x1_q" else []) and all(got[k] is None for k in unread)   # a degree f_out does not name
    assert {k for k in ref if k.startswith("m.")} == {f"m.{n}" for n, _ in mod.named_parameters()}       # every parameter
    G.compare({k: v for k, v in got.items() if v is not None}, ref, F32, name, floor)


@pytest.mark.parametrize("name", ["norm_bias", "g1x1_q", "selfint_final"])
def test_the_compute_mode_changes_no_bit(name):
    mod, h, w = layer_setup(name)
    res = []
    for dtype in (torch.bfloat16, torch.float32):
        R.set_compute_dtype(dtype)
        with G.recording(mod):
            got, out = layer_backward(mod, h, w)
        res.append({**{k: v.clone() for k, v in got.items() if v is not None}, **{f"out{d}": o for d, o in out.items()}})
    assert res[0].keys() == res[1].keys() and all(torch.equal(res[0][k], res[1][k]) for k in res[0])


@pytest.mark.parametrize("name", ["norm_bias", "g1x1_q", "selfint_final"])
def test_recording_forward_is_bitwise_unchanged(name):
    mod, h, _ = layer_setup(name)
    mod = mod.to(DEV)
    try:
        hd = {d: x.to(DEV) for d, x in h.items()}
        ref = mod.run(hd)                               # what GSE3Res and SE3Transformer call: run() without a tape
        same = lambda out: out.keys() == ref.keys() and all(torch.equal(out[d].detach(), ref[d]) for d in ref)  # noqa: E731
        plain = mod(hd)                                 # grad mode on, not opted in: nothing records
        assert same(plain) and not any(o.requires_grad for o in plain.values())
        mod.enable_backward()
        out = mod({d: x.clone().requires_grad_() for d, x in hd.items()})
        assert same(out) and all(o.requires_grad for o in out.values())
        with torch.no_grad():                           # opted in, no grad mode: nothing records either
            assert same(mod(hd))
        assert same(mod.run(hd)) and same(mod.run(hd, tape={}))
    finally:
        mod.enable_backward(False)
        mod.to("cpu")


def test_fp16_small_loss_does_not_underflow():
    """a loss scaled by 2^-20 in the fp16 mode: 2^-20 times the gradient, within the same ceiling"""
    R.set_compute_dtype(torch.float16)
    scale = 2.0 ** -20
    for name in ("norm_bias", "selfint_final", "g1x1_final"):
        mod, h, w = layer_setup(name)
        ref, floor = layer_reference(name)
        with G.recording(mod):
            got, _ = layer_backward(mod, h, w, scale=scale)
        assert all(torch.isfinite(g_).all() and g_.abs().max() > 0 for g_ in got.values())
        G.compare({k: v / scale for k, v in got.items()}, ref, F32, name + " x 2^-20", floor)


def test_backward_is_deterministic():
    for name in ("selfint_final", "norm_bias"):
        mod, h, w = layer_setup(name)
        with G.recording(mod):
            res = [{k: v.clone() for k, v in layer_backward(mod, h, w)[0].items()} for _ in range(2)]
        assert res[0].keys() == res[1].keys() and all(torch.equal(res[0][k], res[1][k]) for k in res[0])


# ================================================================================================ the graph attention
ATT = {"h4": (4, {0: 4, 1: 4}, {0: 4, 1: 4}), "h1": (1, {0: 16, 1: 3}, {0: 16, 1: 3})}   # heads, f_key, f_value
SKIP = {0: 8, 1: 3}
NAMES = ("v0", "v1", "k0", "k1", "q0", "q1", "s0", "s1")


def attention_mask():
    """p = 0.3 on (2, 35); node 0 has no incoming edge, node 1 exactly one, node 2 one from every node (itself included)"""
    mask = (torch.rand(B, LR, LR, generator=G.gen(95)) < 0.3).to(torch.uint8)
    mask[:, :, 0] = 0
    mask[:, :, 1] = 0
    mask[:, LR // 2, 1] = 1
    mask[:, :, 2] = 1
    return mask


@functools.lru_cache(maxsize=None)
def attention_setup(cfg, skip):
    """the mask's edge list, the device graph (the keys of structure.build_graph that GMABSE3 reads) and the operands: v, k per
    edge, padded with zeros to the capacity on the device side; q and skip per node"""
    heads, fk, fv = ATT[cfg]
    mask = attention_mask()
    b, i, j = torch.where(mask.bool())
    src, dst = b * LR + i, b * LR + j
    n = src.numel()
    cap = max(64, (n + 63) // 64 * 64)
    _, _, eid, count = ops.edges_from_mask(mask.to(DEV).contiguous(), cap, zero_tail=True)
    assert count.tolist() == [n, n]
    graph = {"eid": eid, "V": V, "L": LR, "cap": cap}
    x = {"v0": randn(n, fv[0], 1, seed=40), "v1": randn(n, fv[1], 3, seed=41), "k0": randn(n, fk[0], 1, seed=42),
         "k1": randn(n, fk[1], 3, seed=43), "q0": randn(V, fk[0], 1, seed=44), "q1": randn(V, fk[1], 3, seed=45)}
    if skip:
        x.update(s0=randn(V, SKIP[0], 1, seed=46), s1=randn(V, SKIP[1], 3, seed=47))
    w = {d: randn(V, fv[d] + (SKIP[d] if skip else 0), 2 * d + 1, seed=48 + d) for d in (0, 1)}
    return graph, (src, dst), n, x, w


def attention_oracle(cfg, skip, src, dst):
    heads, fk, fv = ATT[cfg]

    def fn(P, v0, v1, k0, k1, q0, q1, s0=None, s1=None):
        z = O.gmab({0: v0, 1: v1}, {0: k0, 1: k1}, {0: q0, 1: q1}, fv, fk, heads, src, dst, V)
        return {0: torch.cat([z[0], s0], 1), 1: torch.cat([z[1], s1], 1)} if skip else z   # GCat, as O.gse3res has it
    return fn


@functools.lru_cache(maxsize=None)
def attention_reference(cfg, skip):
    graph, (src, dst), n, x, w = attention_setup(cfg, skip)
    return G.oracle_grads(attention_oracle(cfg, skip, src, dst), {}, x, lambda out: weighted(out, w))[0]


def attention_backward(mod, cfg, skip, scale=1.0):
    """({input name: gradient; the per-edge ones cut to the first n rows}, detached outputs, the device inputs)"""
    graph, _, n, x, w = attention_setup(cfg, skip)

    def dev(name, t):
        if name[0] in "vk":     # per edge: zeros behind the edge count, as the message kernels leave rows they do not own unread
            t = torch.cat([t, torch.zeros(graph["cap"] - n, *t.shape[1:])])
        return t.to(DEV).requires_grad_()
    xs = {name: dev(name, t) for name, t in x.items()}
    out = mod({0: xs["v0"], 1: xs["v1"]}, {0: xs["k0"], 1: xs["k1"]}, {0: xs["q0"], 1: xs["q1"]}, graph,
              {0: xs["s0"], 1: xs["s1"]} if skip else None)
    (weighted(out, w) * scale).backward()
    grads = {name: (t.grad[:n] if name[0] in "vk" else t.grad) for name, t in xs.items()}
    return grads, {d: o.detach() for d, o in out.items()}, xs


@pytest.mark.parametrize("skip", [False, True], ids=["plain", "skip"])
@pytest.mark.parametrize("cfg", list(ATT))
def test_attention_grads_against_oracle(cfg, skip):
    heads, fk, fv = ATT[cfg]
    ref = attention_reference(cfg, skip)
    mod = S.GMABSE3(fv, fk, n_heads=heads)
    with G.recording(mod):
        got, out, xs = attention_backward(mod, cfg, skip)
        graph, _, n, x, w = attention_setup(cfg, skip)
        plain = mod.run({0: xs["v0"].detach(), 1: xs["v1"].detach()}, {0: xs["k0"].detach(), 1: xs["k1"].detach()},
                        {0: xs["q0"].detach(), 1: xs["q1"].detach()}, graph,
                        {0: xs["s0"].detach(), 1: xs["s1"].detach()} if skip else None)
    assert set(got) == set(ref) == set(NAMES[:8 if skip else 6])                     # every input degree
    G.compare(got, ref, F32, f"GMABSE3 {cfg} {'skip' if skip else 'plain'}")
    assert all(torch.equal(out[d], plain[d]) for d in (0, 1))                        # recording changes no forward bit
    if skip:                                                                         # the trailing channels' gradient, bit for bit
        assert torch.equal(got["s0"].cpu(), w[0][:, fv[0]:]) and torch.equal(got["s1"].cpu(), w[1][:, fv[1]:])
    for b_ in range(B):                                                              # in-degree 0 and 1: exact zeros
        for d in (0, 1):
            assert not got[f"q{d}"][b_ * LR].any() and not got[f"q{d}"][b_ * LR + 1].any()
            e = int(graph["eid"][b_, LR // 2, 1])
            assert not got[f"k{d}"][e].any()
            assert torch.equal(got[f"v{d}"][e].cpu(), w[d][b_ * LR + 1, :fv[d]])


def test_attention_is_mode_independent_and_deterministic():
    heads, fk, fv = ATT["h4"]
    mod = S.GMABSE3(fv, fk, n_heads=heads)
    res = []
    for dtype in (torch.bfloat16, torch.float32, torch.float32):
        R.set_compute_dtype(dtype)
        with G.recording(mod):
            got, out, _ = attention_backward(mod, "h4", True)
        res.append({**{k: v.clone() for k, v in got.items()}, "out0": out[0], "out1": out[1]})
    for other in res[1:]:
        assert all(torch.equal(res[0][k], other[k]) for k in res[0])


def test_attention_fp16_small_loss():
    R.set_compute_dtype(torch.float16)
    scale = 2.0 ** -20
    heads, fk, fv = ATT["h1"]
    mod = S.GMABSE3(fv, fk, n_heads=heads)
    with G.recording(mod):
        got, _, _ = attention_backward(mod, "h1", True, scale=scale)
    G.compare({k: v / scale for k, v in got.items()}, attention_reference("h1", True), F32, "GMABSE3 h1 skip x 2^-20")


def test_attention_refuses_a_chain_beyond_1024_before_any_launch():
    """nothing of the graph but its length is looked at: no tensor needs to exist for the refusal"""
    heads, fk, fv = ATT["h4"]
    mod = S.GMABSE3(fv, fk, n_heads=heads).enable_backward()
    graph = {"eid": None, "V": 1025, "L": 1025}
    with pytest.raises(ValueError):
        mod({0: None, 1: None}, {0: None, 1: None}, {0: None, 1: None}, graph)
    with torch.no_grad(), pytest.raises(ValueError):
        mod({0: None, 1: None}, {0: None, 1: None}, {0: None, 1: None}, graph)
