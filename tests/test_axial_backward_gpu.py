"""Backward pass of the pair axial attention (enable_backward on PerformerSelfAttention, FeedForward,
PairUpdateWithAxialAttentionLayer and PairUpdateWithAxialAttention): the three new kernels against float64 CPU, the modules'
gradients against float64 autograd through the CPU oracle (oracle/rf_oracle.py) in the three compute modes, unchanged forward
numbers, dropout replay (finite differences), fp16 small losses, determinism, the refusals, and the full model with the final
axial update and the head trainable.

The modules are held by the ceiling-or-kink-floor rule of tests/grad_oracle.py: the ReLUs of the feature map and of the
feed-forward are the kinks.  The Performer's projection_matrix is a buffer of the state dict: jittered with the rest, and given
no gradient."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import grad_oracle as G  # noqa: E402
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import ops  # noqa: E402
from oracle import rf_oracle as O  # noqa: E402

DEV = "cuda"
MODES, CEIL, UNIT = G.MODES, G.CEIL, G.UNIT
CENTRED = lambda name: "fn.0.weight" in name   # noqa: E731  the 1-D parameters drawn around 1
_restore_mode = G.restore_mode()


def oracle(fn, P, x, w, dtype, seed=0):
    frozen = [k for k in P if k.endswith("projection_matrix")]
    return G.oracle_grads(fn, P, {"x": x}, w, UNIT[dtype], seed, frozen=frozen)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dtype", MODES)
def test_linattn_normalize_bwd_against_cpu(dtype):
    R.set_compute_dtype(dtype)
    g = G.gen(1)
    rows, dh, ld = 300, 64, 80
    num = torch.randn(rows, ld, generator=g)
    num[:, dh] = torch.rand(rows, generator=g) * 4 + 0.5
    gy = torch.randn(rows, dh, generator=g)
    dn = ops.fill(torch.empty(rows, ld, device=DEV, dtype=dtype), 7.0)
    ops.linattn_normalize_bwd(num.to(DEV), ld, gy.to(DEV), dh, dn, ld, rows, dh)
    nd = num.double().requires_grad_()
    out = nd[:, :dh] / nd[:, dh:dh + 1]
    (out * gy.double()).sum().backward()
    ref = nd.grad
    assert G.rel(dn[:, :dh + 1], ref[:, :dh + 1]) < {torch.float32: 1e-6, torch.float16: 1e-3, torch.bfloat16: 8e-3}[dtype]
    assert torch.all(dn[:, dh + 1:].float() == 0)


@pytest.mark.parametrize("dtype", MODES)
def test_relu_feature_bwd_against_cpu(dtype):
    R.set_compute_dtype(dtype)
    g = G.gen(2)
    rows, ld, m = 257, 288, 266
    dphi, z = torch.randn(rows, ld, generator=g), torch.randn(rows, ld, generator=g)
    dz = ops.relu_feature_bwd(dphi.to(DEV), z.to(DEV), m, dtype)
    ref = torch.where(z > 0, dphi, torch.zeros(()))
    ref[:, m:] = 0
    assert G.rel(dz, ref) < {torch.float32: 1e-7, torch.float16: 1e-3, torch.bfloat16: 8e-3}[dtype]
    assert torch.all(dz[:, m:].float() == 0)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_relu_dropout_bwd_against_cpu(dtype, p):
    R.set_compute_dtype(dtype)
    g = G.gen(3)
    n = 4099
    gh, h = torch.randn(n, generator=g), torch.randn(n, generator=g)
    seed, off = 1234, 77
    drop = (p, seed, off) if p > 0 else None
    dh = ops.relu_dropout_bwd(gh.to(DEV), h.to(DEV), dtype, drop)
    mask = ops.dropout(torch.ones(n, device=DEV), p, seed, off).cpu().double() if p > 0 else torch.ones(n, dtype=torch.float64)
    ref = gh.double() * (h > 0).double() * mask
    assert G.rel(dh, ref) < {torch.float32: 1e-7, torch.float16: 1e-3, torch.bfloat16: 8e-3}[dtype]
    if p > 0:
        assert 0 < (mask == 0).sum() < n


# ------------------------------------------------------------------------------------------------ Performer
def _perf_oracle_grads(mod, xn, w, axis, H, dtype):
    def fn(P, xd):
        B, L1, L2, D = xd.shape
        if axis == 2:
            return O.performer_self_attention(P, "a", xd.reshape(B * L1, L2, D), H, True).view(B, L1, L2, D)
        xs = xd.permute(0, 2, 1, 3).reshape(B * L2, L1, D)
        return O.performer_self_attention(P, "a", xs, H, True).view(B, L2, L1, D).permute(0, 2, 1, 3)
    return oracle(fn, G.state(mod, "a"), xn, w, dtype)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("axis", [1, 2])
@pytest.mark.parametrize("Ls", [64, 96, 128, 256])
def test_performer_grads_against_oracle(dtype, axis, Ls):
    R.set_compute_dtype(dtype)
    torch.manual_seed(Ls + axis)
    D, H, B, Lo = 32, 2, 1, 3
    mod = R.PerformerSelfAttention(D, heads=H, generalized_attention=True).to(DEV)
    G.randomize(mod, 5, CENTRED)
    g = G.gen(Ls * 10 + axis)
    shape = (B, Ls, Lo, D) if axis == 1 else (B, Lo, Ls, D)
    xn = (torch.randn(shape, generator=g)).to(dtype).to(DEV)
    w = torch.randn(shape, generator=g)
    tape = {}
    out = ops.zeros(*shape, device=DEV, dtype=torch.float32)
    mod.attend(xn, out, axis, tape=tape)
    dxn, grads = mod._backward(tape, w.to(DEV).clone())
    ref, floor = _perf_oracle_grads(mod, xn, w, axis, H, dtype)
    got = dict({"a." + name: grads[p] for name, p in mod.named_parameters()}, x=dxn)
    G.compare(got, ref, dtype, f"Performer axis {axis} L={Ls}", floor)
    assert "fast_attention.projection_matrix" not in dict(mod.named_parameters())


@pytest.mark.parametrize("dtype", MODES)
def test_performer_module_forward_autograd(dtype):
    """the public call surface: forward() under grad mode, loss.backward() fills .grad of the parameters and the input"""
    R.set_compute_dtype(dtype)
    torch.manual_seed(9)
    D, H = 32, 2
    mod = R.PerformerSelfAttention(D, heads=H, generalized_attention=True).to(DEV).enable_backward()
    G.randomize(mod, 6, CENTRED)
    g = G.gen(9)
    x = torch.randn(3, 96, D, generator=g).to(dtype).float()
    w = torch.randn(3, 96, D, generator=g)
    got, _ = G.grads_of(mod, {"x": x}, w, pre="a")
    ref, floor = _perf_oracle_grads(mod, x.view(1, 3, 96, D), w.view(1, 3, 96, D), 2, H, dtype)
    G.compare(dict(got, x=got["x"].view(1, 3, 96, D)), ref, dtype, "Performer forward()", floor)


# ------------------------------------------------------------------------------------------------ feed-forward
@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("D,hidden,L", [(288, 1152, 128), (64, 96, 24)])
def test_feed_forward_grads_against_oracle(dtype, D, hidden, L):
    R.set_compute_dtype(dtype)
    torch.manual_seed(D)
    ff = R.FeedForward(D, hidden).to(DEV).enable_backward()
    G.randomize(ff, 7, CENTRED)
    g = G.gen(D + L)
    x = torch.randn(1, L, L, D, generator=g).to(dtype).float()
    w = torch.randn(1, L, L, D, generator=g)
    if D == 288 and dtype != torch.float32:
        assert ops.ffn_fused_applies(x.to(dtype).to(DEV), x.to(DEV), D, hidden)   # the fused forward is what recorded
    got, _ = G.grads_of(ff, {"x": x}, w, pre="ff")
    ref, floor = oracle(lambda P, xd: O.feed_forward(P, "ff", xd), G.state(ff, "ff"), x, w, dtype)
    G.compare(got, ref, dtype, f"FeedForward {D}x{hidden} L={L}", floor)


# ------------------------------------------------------------------------------------------------ layer and stack
@functools.lru_cache(maxsize=None)
def _stack_module(D, H, n_layers, L, seed):
    """module (fp32 weights, CPU), input and output weights (shared by the three modes)"""
    torch.manual_seed(seed)
    if n_layers == 0:
        mod = R.PairUpdateWithAxialAttentionLayer(D, 4 * D, H, 0.1, {})
    else:
        mod = R.PairUpdateWithAxialAttention(D, 4 * D, H, 0.1, n_layers)
    G.randomize(mod, seed, CENTRED)
    g = G.gen(seed)
    return mod, torch.randn(1, L, L, D, generator=g), torch.randn(1, L, L, D, generator=g)


def _check_stack(dtype, D, H, n_layers, L, seed):
    R.set_compute_dtype(dtype)
    mod, x, w = _stack_module(D, H, n_layers, L, seed)
    if n_layers == 0:
        fn = lambda P, xd: O.pair_axial_layer(P, "m", xd, H)   # noqa: E731
    else:
        fn = lambda P, xd: O.pair_update_with_axial_attention(P, "m", xd, n_layers)   # noqa: E731
    ref, floor = oracle(fn, G.state(mod), x, w, dtype, seed)
    mod = mod.to(DEV)
    mod.enable_backward()
    try:
        got, _ = G.grads_of(mod, {"x": x}, w)
        assert set(got) == set(ref) and all(t is not None for t in got.values())
        G.compare(got, ref, dtype, f"axial D={D} layers={n_layers} L={L}", floor)
    finally:
        mod.enable_backward(False)


@pytest.mark.parametrize("dtype", MODES)
def test_axial_layer_grads_against_oracle(dtype):
    _check_stack(dtype, 64, 2, 0, 24, 11)


@pytest.mark.parametrize("dtype", MODES)
def test_axial_stack_grads_against_oracle(dtype):
    _check_stack(dtype, 32, 8, 2, 24, 12)   # (the oracle's stack has 8 heads)


@pytest.mark.parametrize("dtype", [torch.bfloat16])
def test_axial_stack_production_dims(dtype):
    """d_pair 288, 8 heads, 4 layers, L = 128 in the default mode: the fused FAVOR+ / feed-forward / LayerNorm-epilogue forward
    paths record"""
    _check_stack(dtype, 288, 8, 4, 128, 13)


# ------------------------------------------------------------------------------------------------ forward unchanged
@pytest.mark.parametrize("dtype", MODES)
def test_recording_forward_is_bitwise_unchanged(dtype):
    R.set_compute_dtype(dtype)
    torch.manual_seed(21)
    mod = R.PairUpdateWithAxialAttention(288, 1152, 8, 0.1, 2).to(DEV)
    x = torch.randn(1, 128, 128, 288, generator=G.gen(21)).to(DEV)
    with torch.no_grad():
        ref = mod(x)
    mod.enable_backward()
    out = mod(x.clone().requires_grad_())
    assert out.requires_grad and torch.equal(out.detach(), ref)
    layer = mod.layers[0]
    with torch.no_grad():
        ref1 = layer(x)
    assert torch.equal(layer(x.clone().requires_grad_()).detach(), ref1)


# ------------------------------------------------------------------------------------------------ training mode
def test_dropout_replay_finite_differences():
    R.set_compute_dtype(torch.float32)
    torch.manual_seed(31)
    D, H, L = 32, 2, 16
    mod = R.PairUpdateWithAxialAttentionLayer(D, 2 * D, H, 0.2, {}).to(DEV)
    G.randomize(mod, 31, CENTRED)
    mod.train().enable_backward()
    g = G.gen(31)
    x = torch.randn(1, L, L, D, generator=g).to(DEV)
    w = torch.randn(1, L, L, D, generator=g).to(DEV)
    v = torch.randn(1, L, L, D, generator=g).to(DEV)

    def loss(xx):
        R.manual_seed(5)
        return (mod(xx) * w).sum()

    with torch.no_grad():
        mod.eval()
        plain = (mod(x) * w).sum()
        mod.train()
        assert not torch.equal(loss(x), plain)   # the dropouts act
    xg = x.clone().requires_grad_()
    for p in mod.parameters():
        p.grad = None
    loss(xg).backward()
    eps = 1e-3   # (small against the ReLU kinks a central difference steps across; fp32 loss noise ~1e-5)
    with torch.no_grad():
        fd = (loss(x + eps * v) - loss(x - eps * v)).item() / (2 * eps)
    an = (xg.grad * v).sum().item()
    assert abs(fd - an) <= 2e-2 * abs(an) + 1e-3, (fd, an)
    wq = mod.col_attn.to_q.weight
    # a unit-variance direction is ~5x the weights' scale: the step is 10x smaller than x's (the difference converges linearly
    # in the step while it crosses feature-map kinks)
    dw = torch.randn(wq.shape, generator=g).to(DEV) * 0.1
    with torch.no_grad():
        w0 = wq.clone()
        wq.copy_(w0 + eps * dw)
        lp = loss(x).item()
        wq.copy_(w0 - eps * dw)
        lm = loss(x).item()
        wq.copy_(w0)
    an_w = (mod.col_attn.to_q.weight.grad * dw).sum().item()
    assert abs((lp - lm) / (2 * eps) - an_w) <= 2e-2 * abs(an_w) + 1e-3


def test_feed_forward_output_drops_replayed():
    """a direct apply_residual call with output dropouts: the recorded masks are replayed"""
    R.set_compute_dtype(torch.float32)
    torch.manual_seed(32)
    ff = R.FeedForward(32, 64, 0.3).to(DEV).train()
    g = G.gen(32)
    x = torch.randn(1, 8, 8, 32, generator=g).to(DEV)
    w = torch.randn(1, 8, 8, 32, generator=g).to(DEV)
    R.manual_seed(3)
    out, tape = torch.zeros_like(x), {}
    ff.apply_residual(x, out, drops=(0.4,), tape=tape)
    dxn, grads = ff._backward(tape, w.clone())
    assert tape["hdrop"] is not None and len(tape["drops"]) == 1

    def f(xx):
        R.manual_seed(3)
        o = torch.zeros_like(xx)
        ff.apply_residual(xx.contiguous(), o, drops=(0.4,))
        return (o * w).sum()

    v = torch.randn(x.shape, generator=g).to(DEV)
    fd = (f(x + 1e-3 * v) - f(x - 1e-3 * v)).item() / 2e-3
    an = (dxn * v).sum().item()
    assert abs(fd - an) <= 2e-2 * abs(an) + 1e-3, (fd, an)


# ------------------------------------------------------------------------------------------------ fp16 small losses
def test_fp16_small_loss_does_not_underflow():
    R.set_compute_dtype(torch.float16)
    torch.manual_seed(41)
    mod = R.PairUpdateWithAxialAttention(64, 256, 2, 0.1, 2).to(DEV).enable_backward()
    G.randomize(mod, 41, CENTRED)
    g = G.gen(41)
    x = torch.randn(1, 24, 24, 64, generator=g).to(DEV)
    w = torch.randn(1, 24, 24, 64, generator=g).to(DEV)
    res = [list(G.grads_of(mod, {"x": x}, w, scale)[0].values()) for scale in (1.0, 1e-6)]
    for a, b in zip(res[0], res[1]):
        assert torch.isfinite(b).all() and b.abs().max() > 0
        assert G.rel(b * 1e6, a) < CEIL[torch.float16]


# ------------------------------------------------------------------------------------------------ determinism
def test_backward_is_deterministic():
    R.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(51)
    mod = R.PairUpdateWithAxialAttention(288, 1152, 8, 0.1, 1).to(DEV).enable_backward()
    g = G.gen(51)
    x = torch.randn(1, 128, 128, 288, generator=g).to(DEV)
    w = torch.randn(1, 128, 128, 288, generator=g).to(DEV)
    res = [[t.clone() for t in G.grads_of(mod, {"x": x}, w)[0].values()] for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*res))


# ------------------------------------------------------------------------------------------------ refusals
def test_row_group_refused():
    R.set_compute_dtype(torch.float32)
    layer = R.PairUpdateWithAxialAttentionLayer(32, 64, 2, 0.1, {}).to(DEV).enable_backward()
    x = torch.randn(1, 8, 8, 32, device=DEV)
    with pytest.raises(NotImplementedError):
        layer.run(x, row_group=object())
    stack = R.PairUpdateWithAxialAttention(32, 64, 2, 0.1, 1).to(DEV).enable_backward()
    with pytest.raises(NotImplementedError):
        stack.run(x, row_group=object())
    with pytest.raises(NotImplementedError):
        layer.run(x, row_group=object(), tape={})


CFG = dict(d_input=21, d_msa=96, d_pair=72, d_node=8, d_edge=8, d_state=8, n_two_track_blocks=1, n_three_track_blocks=1,
           n_encoder_layers=2, max_len=64, n_neighbors=[128], p_dropout=0.1)


def _inputs(L=16):
    g = G.gen(61)
    msa = torch.randint(0, 21, (1, 6, L), generator=g)
    return msa.to(DEV), msa[:, 0].clone().to(DEV), torch.arange(L).unsqueeze(0).to(DEV)


def test_final_axial_without_head_refused():
    R.set_compute_dtype(torch.float32)
    torch.manual_seed(62)
    model = R.RoseTTAFold(**CFG).to(DEV)
    model.final_block.pair_update_with_axial_attention.enable_backward()
    with pytest.raises(ValueError):
        model(*_inputs())
    with torch.no_grad():   # no grad mode: nothing records, nothing to refuse
        model(*_inputs())


# ------------------------------------------------------------------------------------------------ full model
def test_full_model_final_axial_and_head_train():
    R.set_compute_dtype(torch.float32)
    torch.manual_seed(63)
    model = R.RoseTTAFold(**CFG).to(DEV)
    inp = _inputs()
    with torch.no_grad():
        ref_logits, ref_xyz, ref_plddt = model(*inp)
    axial = model.final_block.pair_update_with_axial_attention
    model.prediction_head.enable_backward()
    axial.enable_backward()
    logits, xyz, plddt = model(*inp)
    for k in ref_logits:
        assert torch.equal(logits[k].detach(), ref_logits[k]), k
    assert torch.equal(xyz, ref_xyz) and torch.equal(plddt, ref_plddt)
    target = {k: torch.randint(0, v.shape[-1], v.shape[:-1], generator=G.gen(64)).to(DEV) for k, v in ref_logits.items()}

    def loss_of(lg):
        return sum(torch.nn.functional.cross_entropy(lg[k].reshape(-1, lg[k].shape[-1]), target[k].reshape(-1)) for k in lg)

    loss_of(logits).backward()
    trainable = {id(p) for p in list(model.prediction_head.parameters()) + list(axial.parameters())}
    for name, p in model.named_parameters():
        assert (p.grad is not None) == (id(p) in trainable), name
    params = [p for p in model.parameters() if id(p) in trainable]
    opt = torch.optim.SGD(params, lr=0.05)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        lv = loss_of(model(*inp)[0])
        losses.append(lv.item())
        lv.backward()
        opt.step()
    with torch.no_grad():
        losses.append(loss_of(model(*inp)[0]).item())
    assert losses[-1] < losses[0], losses
