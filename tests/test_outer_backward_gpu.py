"""Backward pass of OuterProductMean (enable_backward): the fused LayerNorm forward + backward kernel against float64 CPU
autograd, the module's gradients against float64 autograd through the CPU oracle (oracle/rf_oracle.py) in the three compute
modes on every route (general forward, fused forward, several slabs), unchanged forward numbers, the memory bound that "the
P^2-wide tensor never exists" means, determinism, fp16 small losses, the refusals, and the one-input modules the change to
the autograd Function must leave alone."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import ops  # noqa: E402
from rosettafold_pytorch_amd.runtime import RT  # noqa: E402
from oracle import rf_oracle as O  # noqa: E402

DEV = "cuda"
MODES = [torch.float32, torch.bfloat16, torch.float16]
# the rule of tests/test_axial_backward_gpu.py: the mode's ceiling, or three times the float64 gradient's own change under a
# one-rounding-unit relative jitter of inputs and weights, whichever is larger
CEIL = {torch.float32: 1e-4, torch.float16: 1e-2, torch.bfloat16: 5e-2}
UNIT = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
KERNEL_TOL = {torch.float32: 1e-6, torch.float16: 1e-3, torch.bfloat16: 8e-3}   # one pass, one rounding of the result

# (P, Dout, B, N, L): the smallest shape of each route
GENERAL = (4, 16, 2, 5, 7)       # general forward, depth padded to 8, odd L, P % 8 != 0 (the re-laid 16-bit contractions)
FUSED = (32, 288, 1, 64, 16)     # 16-bit modes: the fused forward records
SLABS = (32, 288, 1, 64, 48)     # slab budget forced down: 20 + 20 + 8 rows (16-bit), 10 x 4 + 8 (fp32)
SLAB_BYTES = 20 * 3 * 48 * 1024 * 2


@pytest.fixture(autouse=True)
def _restore_mode():
    budget = RT.outer_bwd_slab_bytes
    yield
    RT.outer_bwd_slab_bytes = budget
    R.set_compute_dtype(torch.bfloat16)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def oracle_grads(fn, P, xs, w, dtype=None, seed=0):
    """float64 autograd of sum(fn(P, **xs) * w): {input name: d/dinput, param name: d/dP[name]}, and with `dtype` also the
    relative change of each under a one-rounding-unit relative jitter of every input and parameter."""
    def run(P, xs):
        P = {k: v.detach().clone().requires_grad_() for k, v in P.items()}
        xd = {k: v.detach().double().cpu().clone().requires_grad_() for k, v in xs.items()}
        (fn(P, **xd) * w.double().cpu()).sum().backward()
        out = {k: v.grad for k, v in P.items() if v.grad is not None}
        out.update({k: v.grad for k, v in xd.items()})
        return out
    ref = run(P, xs)
    if dtype is None:
        return ref, None
    g = gen(seed + 1000)
    jit = lambda t: t * (1 + UNIT[dtype] * (2 * torch.rand(t.shape, generator=g, dtype=torch.float64) - 1))  # noqa: E731
    refj = run({k: jit(v) for k, v in P.items()}, {k: jit(v.detach().double().cpu()) for k, v in xs.items()})
    return ref, {k: rel(refj[k], ref[k]) for k in ref}


def assert_close(got, ref, floor, dtype, key):
    tol = max(CEIL[dtype], 3 * floor[key]) if floor is not None else CEIL[dtype]
    err = rel(got, ref[key])
    print(f"{key}: err {err:.3e} tol {tol:.3e}")
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


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("D", [1024, 16])
def test_layernorm_bwd_fused_against_cpu(dtype, D):
    R.set_compute_dtype(dtype)
    g = gen(D)
    rows, eps = 70, 1e-5   # 70 rows: 8 full blocks of 8 rows and one of 6, its last wave idle
    o = (torch.randn(rows, D, generator=g) * 0.8 + 0.3).to(dtype)
    dz = torch.randn(rows, D, generator=g).to(dtype)
    gamma = torch.randn(D, generator=g) * 0.5 + 1.0
    beta = torch.randn(D, generator=g) * 0.1
    do, z, dgam, dbet = ops.layernorm_bwd_fused(o.to(DEV), dz.to(DEV), gamma.to(DEV), beta.to(DEV), eps=eps)
    assert do.dtype == dtype and z.dtype == dtype
    od, gd, bd = o.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    zr = torch.nn.functional.layer_norm(od, (D,), gd, bd, eps)
    (zr * dz.double()).sum().backward()   # (from the same rounded o and dz the kernel read)
    tol = KERNEL_TOL[dtype]
    for name, got, ref in (("do", do, od.grad), ("z", z, zr), ("dgamma", dgam, gd.grad), ("dbeta", dbet, bd.grad)):
        err = rel(got, ref)
        print(f"{name}: err {err:.3e} tol {tol:.3e}")
        assert err < tol, (name, err, tol)
    # in place (dx over g, z over x) and accumulating: the same bits, and the column sums added to what was there
    oi, di = o.to(DEV), dz.to(DEV)
    acc_g, acc_b = dgam.clone(), dbet.clone()
    ops.layernorm_bwd_fused(oi, di, gamma.to(DEV), beta.to(DEV), eps=eps, dx=di, z=oi, dgamma=acc_g, dbeta=acc_b)
    assert torch.equal(di, do) and torch.equal(oi, z)
    assert torch.equal(acc_g, dgam + dgam) and torch.equal(acc_b, dbet + dbet)


def test_layernorm_bwd_fused_argument_checks():
    R.set_compute_dtype(torch.bfloat16)
    x = torch.zeros(4, 16, device=DEV, dtype=torch.bfloat16)
    gb = torch.ones(16, device=DEV)
    with pytest.raises(ValueError):
        ops.layernorm_bwd_fused(x, x.float(), gb, gb)            # one dtype
    with pytest.raises(ValueError):
        ops.layernorm_bwd_fused(x, x[:, :8], gb, gb)             # one shape, contiguous
    with pytest.raises(ValueError):
        ops.layernorm_bwd_fused(x, x, gb, gb, dgamma=gb.clone())  # both accumulators or neither
    with pytest.raises(R._lib.RfmiError):
        ops.layernorm_bwd_fused(x[:, :12].contiguous(), x[:, :12].contiguous(), gb[:12].contiguous(), gb[:12].contiguous())


# ------------------------------------------------------------------------------------------------ the module
@functools.lru_cache(maxsize=None)
def _case(shape):
    """module (fp32 weights, CPU), x ~ randn, y ~ 0.1 randn, output weights: shared by the modes and the tests"""
    P, Dout, B, N, L = shape
    torch.manual_seed(P + L)
    mod = randomize(R.OuterProductMean(P, Dout), L)
    g = gen(L)
    return (mod, torch.randn(B, N, L, P, generator=g), 0.1 * torch.randn(B, N, L, P, generator=g),
            torch.randn(B, L, L, Dout, generator=g))


@functools.lru_cache(maxsize=None)
def _reference(shape, dtype, one):
    """float64 oracle gradients of the operands as the mode holds them (rounded to its operand type), and the jitter floor"""
    mod, x, y, w = _case(shape)
    x, y = x.to(dtype).float(), y.to(dtype).float()
    if one:
        return oracle_grads(lambda P, x: O.outer_product_mean(P, "m", x, x), state(mod, "m"), {"x": x}, w, dtype)
    return oracle_grads(lambda P, x, y: O.outer_product_mean(P, "m", x, y), state(mod, "m"), {"x": x, "y": y}, w, dtype)


def _slabs(mod, shape):
    h = mod.backward_slab_rows(shape[4], shape[0])
    return -(-shape[4] // h), shape[4] % h


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("one", [False, True], ids=["xy", "x"])
@pytest.mark.parametrize("shape", [GENERAL, FUSED, SLABS], ids=["general", "fused", "slabs"])
def test_module_grads_against_oracle(dtype, one, shape):
    R.set_compute_dtype(dtype)
    cpu_mod, x, y, w = _case(shape)
    ref, floor = _reference(shape, dtype, one)
    P, Dout, B, N, L = shape
    mod = R.OuterProductMean(P, Dout)
    mod.load_state_dict(cpu_mod.state_dict())
    mod = mod.to(DEV).enable_backward()
    if shape == FUSED and dtype != torch.float32:
        assert mod.fused_ok(P, N, L)   # the fused forward is what recorded
    if shape == SLABS:
        RT.outer_bwd_slab_bytes = SLAB_BYTES
        n, ragged = _slabs(mod, shape)
        assert n >= 3 and ragged, (n, ragged)
    else:
        assert _slabs(mod, shape) == (1, 0)
    xg = x.to(dtype).float().to(DEV).requires_grad_()
    yg = y.to(dtype).float().to(DEV).requires_grad_()
    out = mod(xg) if one else mod(xg, yg)
    (out * w.to(DEV)).sum().backward()
    assert_close(xg.grad, ref, floor, dtype, "x")
    if one:
        assert yg.grad is None
    else:
        assert_close(yg.grad, ref, floor, dtype, "y")
    assert {"m." + n_ for n_, _ in mod.named_parameters()} | ({"x"} if one else {"x", "y"}) == set(ref)
    for name, p in mod.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape
        assert_close(p.grad, ref, floor, dtype, "m." + name)


def test_only_the_wanted_input_gets_a_gradient():
    R.set_compute_dtype(torch.float32)
    cpu_mod, x, y, w = _case(GENERAL)
    ref, _ = _reference(GENERAL, torch.float32, False)
    mod = R.OuterProductMean(GENERAL[0], GENERAL[1])
    mod.load_state_dict(cpu_mod.state_dict())
    mod = mod.to(DEV).enable_backward()
    xg, yg = x.to(DEV), y.to(DEV).requires_grad_()
    (mod(xg, yg) * w.to(DEV)).sum().backward()
    assert xg.grad is None
    assert_close(yg.grad, ref, None, torch.float32, "y")


# ------------------------------------------------------------------------------------------------ forward unchanged
@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("shape", [GENERAL, FUSED], ids=["general", "fused"])
def test_recording_forward_is_bitwise_unchanged(dtype, shape):
    R.set_compute_dtype(dtype)
    cpu_mod, x, y, _ = _case(shape)
    mod = R.OuterProductMean(shape[0], shape[1])
    mod.load_state_dict(cpu_mod.state_dict())
    mod = mod.to(DEV)
    x, y = x.to(DEV), y.to(DEV)
    with torch.no_grad():
        ref, ref1 = mod(x, y), mod(x)
    mod.enable_backward()
    out = mod(x.clone().requires_grad_(), y.clone().requires_grad_())
    assert out.requires_grad and torch.equal(out.detach(), ref)
    assert torch.equal(mod(x.clone().requires_grad_()).detach(), ref1)
    with torch.no_grad():
        assert torch.equal(mod(x, y), ref)


# ------------------------------------------------------------------------------------------------ memory
def test_backward_never_holds_the_wide_tensor():
    """B = 1, L = 128, N = 64, P = 32, Dout = 288, bf16, default slab budget: what backward() allocates on top of what was
    live before it stays below half of one fp32 [B, L, L, P^2] tensor (33.5 MB).  The output gradient is handed to backward(),
    so the figure holds the module's own allocations and not autograd's product out * w."""
    R.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(71)
    B, L, N, P, Dout = 1, 128, 64, 32, 288
    mod = R.OuterProductMean(P, Dout).to(DEV).enable_backward()
    g = gen(71)
    x = torch.randn(B, N, L, P, generator=g).to(DEV).requires_grad_()
    y = (0.1 * torch.randn(B, N, L, P, generator=g)).to(DEV).requires_grad_()
    w = torch.randn(B, L, L, Dout, generator=g).to(DEV)
    out = mod(x, y)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out.backward(w)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    bound = B * L * L * P * P * 4 // 2
    print(f"peak extra {extra / 1e6:.1f} MB, bound {bound / 1e6:.1f} MB")
    assert x.grad is not None and y.grad is not None
    assert extra < bound, (extra, bound)


# ------------------------------------------------------------------------------------------------ determinism
def test_backward_is_deterministic():
    R.set_compute_dtype(torch.bfloat16)
    RT.outer_bwd_slab_bytes = SLAB_BYTES
    cpu_mod, x, y, w = _case(SLABS)
    mod = R.OuterProductMean(SLABS[0], SLABS[1])
    mod.load_state_dict(cpu_mod.state_dict())
    mod = mod.to(DEV).enable_backward()
    assert _slabs(mod, SLABS)[0] >= 3
    res = []
    for _ in range(2):
        for p in mod.parameters():
            p.grad = None
        xg, yg = x.to(DEV).requires_grad_(), y.to(DEV).requires_grad_()
        (mod(xg, yg) * w.to(DEV)).sum().backward()
        res.append([xg.grad.clone(), yg.grad.clone()] + [p.grad.clone() for p in mod.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*res))


# ------------------------------------------------------------------------------------------------ fp16 small losses
def test_fp16_small_loss_does_not_underflow():
    R.set_compute_dtype(torch.float16)
    cpu_mod, x, y, w = _case(FUSED)
    mod = R.OuterProductMean(FUSED[0], FUSED[1])
    mod.load_state_dict(cpu_mod.state_dict())
    mod = mod.to(DEV).enable_backward()
    res = []
    for scale in (1.0, 1e-6):
        for p in mod.parameters():
            p.grad = None
        xg, yg = x.to(DEV).requires_grad_(), y.to(DEV).requires_grad_()
        ((mod(xg, yg) * w.to(DEV)).sum() * scale).backward()
        res.append([xg.grad, yg.grad] + [p.grad for p in mod.parameters()])
    for a, b in zip(res[0], res[1]):
        assert torch.isfinite(b).all() and b.abs().max() > 0
        assert rel(b * 1e6, a) < CEIL[torch.float16]


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    R.set_compute_dtype(torch.float32)
    mod = R.OuterProductMean(4, 16).to(DEV).enable_backward()
    x = torch.randn(1, 5, 7, 4, device=DEV)
    xt, yt, Np = ops.outer_operands(x, x, torch.float32)
    with pytest.raises(NotImplementedError):
        mod.run_rows(xt[:, :3].contiguous(), yt, Np)
    odd = R.OuterProductMean(3, 16).to(DEV).enable_backward()
    x3 = torch.randn(1, 5, 7, 3, device=DEV)
    with pytest.raises(ValueError):
        odd(x3)
    with torch.no_grad():   # no grad mode: nothing records, nothing is refused
        assert odd(x3).shape == (1, 7, 7, 16) and not odd(x3).requires_grad
        assert mod.run_rows(xt[:, :3].contiguous(), yt, Np).shape == (1, 3, 7, 16)


# ------------------------------------------------------------------------------------------------ one-input modules
def test_one_input_modules_unchanged():
    """FeedForward and the generalized Performer go through the same autograd Function as before: gradients of the input and
    of every parameter, the same bits on a second run"""
    R.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(81)
    g = gen(81)
    for mod, shape in ((R.FeedForward(64, 96), (1, 8, 8, 64)),
                       (R.PerformerSelfAttention(32, heads=2, generalized_attention=True), (3, 64, 32))):
        mod = randomize(mod.to(DEV), 81).enable_backward()
        x, w = torch.randn(shape, generator=g).to(DEV), torch.randn(shape, generator=g).to(DEV)
        res = []
        for _ in range(2):
            for p in mod.parameters():
                p.grad = None
            xg = x.clone().requires_grad_()
            (mod(xg) * w).sum().backward()
            assert xg.grad.shape == x.shape and all(p.grad is not None for p in mod.parameters())
            res.append([xg.grad.clone()] + [p.grad.clone() for p in mod.parameters()])
        assert all(torch.equal(a, b) for a, b in zip(*res))
        assert all(torch.isfinite(t).all() and t.abs().max() > 0 for t in res[0])
