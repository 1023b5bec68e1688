"""Backward pass of the pair axial attention (enable_backward on PerformerSelfAttention, FeedForward,
PairUpdateWithAxialAttentionLayer and PairUpdateWithAxialAttention): the three new kernels against float64 CPU, the modules'
gradients against float64 autograd through the CPU oracle (oracle/rf_oracle.py) in the three compute modes, unchanged forward
numbers, dropout replay (finite differences), fp16 small losses, determinism, the refusals, and the full model with the final
axial update and the head trainable."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import ops  # noqa: E402
from oracle import rf_oracle as O  # noqa: E402

DEV = "cuda"
MODES = [torch.float32, torch.bfloat16, torch.float16]
CEIL = {torch.float32: 1e-4, torch.float16: 1e-2, torch.bfloat16: 5e-2}


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    R.set_compute_dtype(torch.bfloat16)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def gen(seed):
    return torch.Generator().manual_seed(seed)


# Rounding unit of each mode's 16-bit / fp32 operands.  The ReLUs (feature map, feed-forward) make the exact gradient a
# discontinuous function of the forward's values: wherever a pre-activation lies within rounding distance of 0 the forward of
# that mode may take the other side of the kink.  The oracle comparison therefore allows, besides the mode's ceiling, three
# times the float64 gradient's own change under a relative perturbation of its inputs and weights of one rounding unit.
UNIT = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def oracle_grads(fn, P, x, w, dtype=None, seed=0):
    """float64 autograd of sum(fn(P, x) * w): {"x": d/dx, name: d/dP[name]}, and with `dtype` also the same after a
    one-rounding-unit relative jitter of x and every parameter (the kink floor, see UNIT)."""
    def run(P, x):
        P = {k: v.detach().clone().requires_grad_(not k.endswith("projection_matrix")) for k, v in P.items()}
        xd = x.detach().double().cpu().clone().requires_grad_()
        (fn(P, xd) * w.double().cpu()).sum().backward()
        out = {k: v.grad for k, v in P.items() if v.grad is not None}
        out["x"] = xd.grad
        return out
    ref = run(P, x)
    if dtype is None:
        return ref, None
    g = gen(seed + 1000)
    jit = lambda t: t * (1 + UNIT[dtype] * (2 * torch.rand(t.shape, generator=g, dtype=torch.float64) - 1))  # noqa: E731
    refj = run({k: jit(v) for k, v in P.items()}, jit(x.detach().double().cpu()))
    return ref, {k: rel(refj[k], ref[k]) for k in ref}


def assert_close(got, ref, floor, dtype, key):
    tol = max(CEIL[dtype], 3 * floor[key]) if floor is not None else CEIL[dtype]
    err = rel(got, ref[key])
    assert err < tol, (key, err, tol)


def state(mod, pre):
    return {f"{pre}.{k}": v.detach().double().cpu() for k, v in mod.state_dict().items()}


def randomize(mod, seed):
    """non-trivial LayerNorm affines and biases (the defaults 1 / 0 would hide their gradients' mistakes)"""
    g = gen(seed)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if p.dim() == 1:
                p.copy_((torch.randn(p.shape, generator=g) * 0.1 + (1.0 if "fn.0.weight" in name else 0.0)).to(p.device))
    return mod


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dtype", MODES)
def test_linattn_normalize_bwd_against_cpu(dtype):
    R.set_compute_dtype(dtype)
    g = gen(1)
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
    assert rel(dn[:, :dh + 1], ref[:, :dh + 1]) < {torch.float32: 1e-6, torch.float16: 1e-3, torch.bfloat16: 8e-3}[dtype]
    assert torch.all(dn[:, dh + 1:].float() == 0)


@pytest.mark.parametrize("dtype", MODES)
def test_relu_feature_bwd_against_cpu(dtype):
    R.set_compute_dtype(dtype)
    g = gen(2)
    rows, ld, m = 257, 288, 266
    dphi, z = torch.randn(rows, ld, generator=g), torch.randn(rows, ld, generator=g)
    dz = ops.relu_feature_bwd(dphi.to(DEV), z.to(DEV), m, dtype)
    ref = torch.where(z > 0, dphi, torch.zeros(()))
    ref[:, m:] = 0
    assert rel(dz, ref) < {torch.float32: 1e-7, torch.float16: 1e-3, torch.bfloat16: 8e-3}[dtype]
    assert torch.all(dz[:, m:].float() == 0)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_relu_dropout_bwd_against_cpu(dtype, p):
    R.set_compute_dtype(dtype)
    g = gen(3)
    n = 4099
    gh, h = torch.randn(n, generator=g), torch.randn(n, generator=g)
    seed, off = 1234, 77
    drop = (p, seed, off) if p > 0 else None
    dh = ops.relu_dropout_bwd(gh.to(DEV), h.to(DEV), dtype, drop)
    mask = ops.dropout(torch.ones(n, device=DEV), p, seed, off).cpu().double() if p > 0 else torch.ones(n, dtype=torch.float64)
    ref = gh.double() * (h > 0).double() * mask
    assert rel(dh, ref) < {torch.float32: 1e-7, torch.float16: 1e-3, torch.bfloat16: 8e-3}[dtype]
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
    return oracle_grads(fn, state(mod, "a"), xn, w, dtype)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("axis", [1, 2])
@pytest.mark.parametrize("Ls", [64, 96, 128, 256])
def test_performer_grads_against_oracle(dtype, axis, Ls):
    R.set_compute_dtype(dtype)
    torch.manual_seed(Ls + axis)
    D, H, B, Lo = 32, 2, 1, 3
    mod = R.PerformerSelfAttention(D, heads=H, generalized_attention=True).to(DEV)
    randomize(mod, 5)
    g = gen(Ls * 10 + axis)
    shape = (B, Ls, Lo, D) if axis == 1 else (B, Lo, Ls, D)
    xn = (torch.randn(shape, generator=g)).to(dtype).to(DEV)
    w = torch.randn(shape, generator=g)
    tape = {}
    out = ops.zeros(*shape, device=DEV, dtype=torch.float32)
    mod.attend(xn, out, axis, tape=tape)
    dxn, grads = mod._backward(tape, w.to(DEV).clone())
    ref, floor = _perf_oracle_grads(mod, xn, w, axis, H, dtype)
    assert_close(dxn, ref, floor, dtype, "x")
    for name, p in mod.named_parameters():
        assert_close(grads[p], ref, floor, dtype, "a." + name)
    assert "fast_attention.projection_matrix" not in dict(mod.named_parameters())


@pytest.mark.parametrize("dtype", MODES)
def test_performer_module_forward_autograd(dtype):
    """the public call surface: forward() under grad mode, loss.backward() fills .grad of the parameters and the input"""
    R.set_compute_dtype(dtype)
    torch.manual_seed(9)
    D, H = 32, 2
    mod = R.PerformerSelfAttention(D, heads=H, generalized_attention=True).to(DEV).enable_backward()
    randomize(mod, 6)
    g = gen(9)
    x = torch.randn(3, 96, D, generator=g).to(dtype).float()
    w = torch.randn(3, 96, D, generator=g)
    xg = x.to(DEV).requires_grad_()
    (mod(xg) * w.to(DEV)).sum().backward()
    ref, floor = _perf_oracle_grads(mod, x.view(1, 3, 96, D), w.view(1, 3, 96, D), 2, H, dtype)
    assert_close(xg.grad.view(1, 3, 96, D), ref, floor, dtype, "x")
    for name, p in mod.named_parameters():
        assert_close(p.grad, ref, floor, dtype, "a." + name)


# ------------------------------------------------------------------------------------------------ feed-forward
@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("D,hidden,L", [(288, 1152, 128), (64, 96, 24)])
def test_feed_forward_grads_against_oracle(dtype, D, hidden, L):
    R.set_compute_dtype(dtype)
    torch.manual_seed(D)
    ff = R.FeedForward(D, hidden).to(DEV).enable_backward()
    randomize(ff, 7)
    g = gen(D + L)
    x = torch.randn(1, L, L, D, generator=g).to(dtype).float()
    w = torch.randn(1, L, L, D, generator=g)
    if D == 288 and dtype != torch.float32:
        assert ops.ffn_fused_applies(x.to(dtype).to(DEV), x.to(DEV), D, hidden)   # the fused forward is what recorded
    xg = x.to(DEV).requires_grad_()
    (ff(xg) * w.to(DEV)).sum().backward()
    ref, floor = oracle_grads(lambda P, xd: O.feed_forward(P, "ff", xd), state(ff, "ff"), x, w, dtype)
    assert_close(xg.grad, ref, floor, dtype, "x")
    for name, p in ff.named_parameters():
        assert_close(p.grad, ref, floor, dtype, "ff." + name)


# ------------------------------------------------------------------------------------------------ layer and stack
@functools.lru_cache(maxsize=None)
def _stack_module(D, H, n_layers, L, seed):
    """module (fp32 weights, CPU), input and output weights (shared by the three modes)"""
    torch.manual_seed(seed)
    if n_layers == 0:
        mod = R.PairUpdateWithAxialAttentionLayer(D, 4 * D, H, 0.1, {})
    else:
        mod = R.PairUpdateWithAxialAttention(D, 4 * D, H, 0.1, n_layers)
    randomize(mod, seed)
    g = gen(seed)
    return mod, torch.randn(1, L, L, D, generator=g), torch.randn(1, L, L, D, generator=g)


def _check_stack(dtype, D, H, n_layers, L, seed):
    R.set_compute_dtype(dtype)
    mod, x, w = _stack_module(D, H, n_layers, L, seed)
    if n_layers == 0:
        fn = lambda P, xd: O.pair_axial_layer(P, "m", xd, H)   # noqa: E731
    else:
        fn = lambda P, xd: O.pair_update_with_axial_attention(P, "m", xd, n_layers)   # noqa: E731
    ref, floor = oracle_grads(fn, state(mod, "m"), x, w, dtype, seed)
    mod = mod.to(DEV)
    mod.enable_backward()
    try:
        for p in mod.parameters():
            p.grad = None
        xg = x.to(DEV).requires_grad_()
        (mod(xg) * w.to(DEV)).sum().backward()
        assert_close(xg.grad, ref, floor, dtype, "x")
        assert {"m." + n for n, _ in mod.named_parameters()} | {"x"} == set(ref)
        for name, p in mod.named_parameters():
            assert p.grad is not None
            assert_close(p.grad, ref, floor, dtype, "m." + name)
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
    x = torch.randn(1, 128, 128, 288, generator=gen(21)).to(DEV)
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
    randomize(mod, 31)
    mod.train().enable_backward()
    g = gen(31)
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
    g = gen(32)
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
    randomize(mod, 41)
    g = gen(41)
    x = torch.randn(1, 24, 24, 64, generator=g).to(DEV)
    w = torch.randn(1, 24, 24, 64, generator=g).to(DEV)
    res = []
    for scale in (1.0, 1e-6):
        for p in mod.parameters():
            p.grad = None
        xg = x.clone().requires_grad_()
        ((mod(xg) * w).sum() * scale).backward()
        res.append([xg.grad] + [p.grad for p in mod.parameters()])
    for a, b in zip(res[0], res[1]):
        assert torch.isfinite(b).all() and b.abs().max() > 0
        assert rel(b * 1e6, a) < CEIL[torch.float16]


# ------------------------------------------------------------------------------------------------ determinism
def test_backward_is_deterministic():
    R.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(51)
    mod = R.PairUpdateWithAxialAttention(288, 1152, 8, 0.1, 1).to(DEV).enable_backward()
    g = gen(51)
    x = torch.randn(1, 128, 128, 288, generator=g).to(DEV)
    w = torch.randn(1, 128, 128, 288, generator=g).to(DEV)
    res = []
    for _ in range(2):
        for p in mod.parameters():
            p.grad = None
        xg = x.clone().requires_grad_()
        (mod(xg) * w).sum().backward()
        res.append([xg.grad.clone()] + [p.grad.clone() for p in mod.parameters()])
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
    g = gen(61)
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
    target = {k: torch.randint(0, v.shape[-1], v.shape[:-1], generator=gen(64)).to(DEV) for k, v in ref_logits.items()}

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
