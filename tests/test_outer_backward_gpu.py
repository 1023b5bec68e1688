"""Backward pass of OuterProductMean (enable_backward): the fused LayerNorm forward + backward kernel against float64 CPU
autograd, the module's gradients against float64 autograd through the CPU oracle (oracle/rf_oracle.py) in the three compute
modes on every route (general forward, fused forward, several slabs), unchanged forward numbers, the memory bound that "the
P^2-wide tensor never exists" means, determinism, fp16 small losses, the refusals, and the one-input modules the change to
the autograd Function must leave alone.  The module is held by the ceiling-or-kink-floor rule of tests/grad_oracle.py."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import grad_oracle as G  # noqa: E402
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import ops  # noqa: E402
from rosettafold_pytorch_amd.runtime import RT  # noqa: E402
from oracle import rf_oracle as O  # noqa: E402

DEV = "cuda"
MODES, CEIL, UNIT = G.MODES, G.CEIL, G.UNIT
KERNEL_TOL = {torch.float32: 1e-6, torch.float16: 1e-3, torch.bfloat16: 8e-3}   # one pass, one rounding of the result

# (P, Dout, B, N, L): the smallest shape of each route
GENERAL = (4, 16, 2, 5, 7)       # general forward, depth padded to 8, odd L, P % 8 != 0 (the re-laid 16-bit contractions)
FUSED = (32, 288, 1, 64, 16)     # 16-bit modes: the fused forward records
SLABS = (32, 288, 1, 64, 48)     # slab budget forced down: 20 + 20 + 8 rows (16-bit), 10 x 4 + 8 (fp32)
SLAB_BYTES = 20 * 3 * 48 * 1024 * 2
CENTRED = lambda name: "fn.0.weight" in name   # noqa: E731  the 1-D parameters drawn around 1
_restore_mode = G.restore_mode(also=(RT, "outer_bwd_slab_bytes"))


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("D", [1024, 16])
def test_layernorm_bwd_fused_against_cpu(dtype, D):
    R.set_compute_dtype(dtype)
    g = G.gen(D)
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
        err = G.rel(got, ref)
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
    mod = G.randomize(R.OuterProductMean(P, Dout), L, CENTRED)
    g = G.gen(L)
    return (mod, torch.randn(B, N, L, P, generator=g), 0.1 * torch.randn(B, N, L, P, generator=g),
            torch.randn(B, L, L, Dout, generator=g))


@functools.lru_cache(maxsize=None)
def _reference(shape, dtype, one):
    """float64 oracle gradients of the operands as the mode holds them (rounded to its operand type), and the jitter floor"""
    mod, x, y, w = _case(shape)
    x, y = x.to(dtype).float(), y.to(dtype).float()
    if one:
        return G.oracle_grads(lambda P, x: O.outer_product_mean(P, "m", x, x), G.state(mod), {"x": x}, w, UNIT[dtype])
    return G.oracle_grads(lambda P, x, y: O.outer_product_mean(P, "m", x, y), G.state(mod), {"x": x, "y": y}, w, UNIT[dtype])


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
    xs = {"x": x.to(dtype).float()} if one else {"x": x.to(dtype).float(), "y": y.to(dtype).float()}
    got, _ = G.grads_of(mod, xs, w)
    assert set(got) == set(ref)
    for name, p in mod.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape
    G.compare(got, ref, dtype, f"{shape} {'x' if one else 'xy'}", floor)


def test_only_the_wanted_input_gets_a_gradient():
    R.set_compute_dtype(torch.float32)
    cpu_mod, x, y, w = _case(GENERAL)
    ref, _ = _reference(GENERAL, torch.float32, False)
    mod = R.OuterProductMean(GENERAL[0], GENERAL[1])
    mod.load_state_dict(cpu_mod.state_dict())
    mod = mod.to(DEV).enable_backward()
    xg = x.to(DEV)
    got, _ = G.grads_of(mod, {"x": xg, "y": y}, w, leaves=("y",))
    assert xg.grad is None and "x" not in got
    G.compare(got, {"y": ref["y"]}, torch.float32, f"{GENERAL} y alone")


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
    g = G.gen(71)
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
    res = [[t.clone() for t in G.grads_of(mod, {"x": x, "y": y}, w)[0].values()] for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*res))


# ------------------------------------------------------------------------------------------------ fp16 small losses
def test_fp16_small_loss_does_not_underflow():
    R.set_compute_dtype(torch.float16)
    cpu_mod, x, y, w = _case(FUSED)
    mod = R.OuterProductMean(FUSED[0], FUSED[1])
    mod.load_state_dict(cpu_mod.state_dict())
    mod = mod.to(DEV).enable_backward()
    res = [list(G.grads_of(mod, {"x": x, "y": y}, w, scale)[0].values()) for scale in (1.0, 1e-6)]
    for a, b in zip(res[0], res[1]):
        assert torch.isfinite(b).all() and b.abs().max() > 0
        assert G.rel(b * 1e6, a) < CEIL[torch.float16]


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
    g = G.gen(81)
    for mod, shape in ((R.FeedForward(64, 96), (1, 8, 8, 64)),
                       (R.PerformerSelfAttention(32, heads=2, generalized_attention=True), (3, 64, 32))):
        mod = G.randomize(mod.to(DEV), 81, CENTRED).enable_backward()
        x, w = torch.randn(shape, generator=g).to(DEV), torch.randn(shape, generator=g).to(DEV)
        res = []
        for _ in range(2):
            got, _ = G.grads_of(mod, {"x": x}, w)
            assert got["x"].shape == x.shape and all(t is not None for t in got.values())
            res.append([t.clone() for t in got.values()])
        assert all(torch.equal(a, b) for a, b in zip(*res))
        assert all(torch.isfinite(t).all() and t.abs().max() > 0 for t in res[0])
