"""The fused outer product (csrc/outer.hip) at any chain length and MSA depth and on rectangular pictures: against float64 on the
same 16-bit operands at the smallest shapes at which a tail tile, the depth padding or a sample boundary can go wrong; bit
equality of a ragged picture with the same pairs inside a picture of whole tiles and of a block of rows with those rows of the
square; nothing written outside the addressed output, nothing read outside the operands; the modules that now take the route
(forward against the CPU oracle, OuterProductMean's backward against the oracle's autograd); determinism."""
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
P, DOUT, LD = 32, 288, 304
DTS = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
TOL_OUT, TOL_LN2 = 1.5e-2, 2e-2   # tests/test_kernels_gpu.py::test_outer_product_fused, bf16; fp16 is held to the same numbers


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    RT.fused_outer = True
    R.set_compute_dtype(torch.bfloat16)


def randn(*s, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(s))
    return torch.randn(*s, generator=g)


def max_err(a, b):
    """what test_outer_product_fused measures: max |a - b| / max |b|"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-20)).item()


def l2_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def close(got, ref, tol, what):
    e2, em = l2_err(got, ref), max_err(got, ref)
    print(f"{what}: rel-L2 {e2:.3e} max-norm {em:.3e} tol {tol:.1e}")
    assert torch.isfinite(got).all(), what
    assert e2 < tol and em < tol, (what, e2, em, tol)


@functools.lru_cache(maxsize=None)
def params():
    """LayerNorm(1024) / Linear / LayerNorm(288) parameters of test_outer_product_fused (fp32, on the host)"""
    g_, b_ = 1.0 + 0.2 * randn(P * P, seed=2), 0.1 * randn(P * P, seed=3)
    w, bias = randn(DOUT, P * P, seed=4) * 0.05, randn(DOUT, seed=5)
    g2, b2 = 1.0 + 0.2 * randn(DOUT, seed=8), 0.1 * randn(DOUT, seed=9)
    return g_, b_, w, bias, g2, b2


@functools.lru_cache(maxsize=None)
def case(B, N, Lr, dt):
    """inputs as test_outer_product_fused builds them, rounded to the 16-bit type, and the float64 reference of both output
    forms from those rounded operands (computed once; nothing mutates it)"""
    x, y = randn(B, N, Lr, P).to(dt), (randn(B, N, Lr, P, seed=1) * 0.3).to(dt)
    g_, b_, w, bias, g2, b2 = params()
    co = torch.einsum("bniu,bnjv->bijuv", x.double(), y.double()).reshape(B, Lr, Lr, P * P)
    F = torch.nn.functional
    ref = F.linear(F.layer_norm(co, (P * P,), g_.double(), b_.double(), 1e-5), w.double(), bias.double())
    ref2 = F.layer_norm(ref, (DOUT,), g2.double(), b2.double(), 1e-5)
    return x.to(DEV), y.to(DEV), ref, ref2


def fold(dt):
    g_, b_, w, bias, g2, b2 = params()
    wp, s_, c_ = ops.outer_fold(w.to(DEV), g_.to(DEV), b_.to(DEV), bias.to(DEV), dt)
    return wp, s_, c_, g2.to(DEV).contiguous(), b2.to(DEV).contiguous()


def operands(x, y, dt):
    """x, y [B, N, L, P] -> transposed operands at the fused kernel's depth"""
    xt, yt, Np = ops.outer_operands(x, y, dt, ops.outer_depth(x.shape[1]))
    assert Np in (64, 128)
    return xt, yt


def fused(xt, yt, dt, form, out=None):
    """one launch: form "out" -> fp32 [B, Li, Lj, 288]; form "y" -> the LN2 image in a [B, Li, Lj, 304] tensor pre-filled with 3"""
    wp, s_, c_, g2, b2 = fold(dt)
    B, Li, Lj = xt.shape[0], xt.shape[1], yt.shape[1]
    if form == "out":
        out = torch.empty(B, Li, Lj, DOUT, device=DEV, dtype=torch.float32) if out is None else out
        return ops.outer_fused(xt, yt, wp, s_, c_, out, 1e-5)
    feat = torch.full((B, Li, Lj, LD), 3.0, device=DEV, dtype=dt) if out is None else out
    ops.outer_fused(xt, yt, wp, s_, c_, None, 1e-5, ln2=(g2, b2, 1e-5, feat, LD))
    return feat


class count_fused:
    """wraps ops.outer_fused and counts the calls (the route is observed, not assumed)"""

    def __enter__(self):
        self.n, self.orig = 0, ops.outer_fused

        def wrapped(*a, **kw):
            self.n += 1
            return self.orig(*a, **kw)
        ops.outer_fused = wrapped
        return self

    def __exit__(self, *exc):
        ops.outer_fused = self.orig


# ------------------------------------------------------------------------------------------------ the kernel against float64
# (B, N, L): one pair; less than a tile either way; a column tail; row and column tails over two samples; a row tail only
# (L % 8 == 0, L % 16 != 0); several tiles with both tails
SHAPES = [(2, 128, 1), (2, 64, 7), (1, 128, 9), (2, 128, 17), (1, 64, 24), (2, 128, 33)]


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("B,N,Lr", SHAPES + [(2, n, 17) for n in (1, 5, 72, 100)], ids=lambda v: str(v))
def test_kernel_against_float64(B, N, Lr, dt):
    R.set_compute_dtype(dt)
    x, y, ref, ref2 = case(B, N, Lr, dt)
    g_, b_, w, bias, _, _ = params()
    # the functional form pads the depth itself (and is what torch.ops.rfmi.outer_product_ln_linear runs)
    out = ops.outer_product_ln_linear(x, y, g_.to(DEV), b_.to(DEV), w.to(DEV), bias.to(DEV), 1e-5)
    assert out.shape == (B, Lr, Lr, DOUT) and out.dtype == torch.float32
    close(out, ref, TOL_OUT, "out")
    xt, yt = operands(x, y, dt)
    assert torch.equal(fused(xt, yt, dt, "out"), out)
    feat = fused(xt, yt, dt, "y")
    close(feat[..., :DOUT].float(), ref2, TOL_LN2, "ln2")
    assert (feat[..., DOUT:] == 3.0).all()


def test_dispatcher_op_takes_ragged_shapes():
    import rosettafold_pytorch_amd.custom_ops  # noqa: F401
    x, y, ref, _ = case(2, 100, 17, torch.bfloat16)
    g_, b_, w, bias, _, _ = params()
    out = torch.ops.rfmi.outer_product_ln_linear(x, y, g_.to(DEV), b_.to(DEV), w.to(DEV), bias.to(DEV), 1e-5)
    close(out, ref, TOL_OUT, "dispatcher")


# ------------------------------------------------------------------------------------------------ bit equality with whole tiles
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("Lr", [9, 17, 33])
@pytest.mark.parametrize("form", ["out", "y"])
def test_ragged_equals_the_full_tile_picture(Lr, form, dt):
    """the pairs of a ragged picture inside a picture of whole tiles whose other residues hold arbitrary finite values: the
    same bits (a pair's arithmetic does not depend on its neighbours, nor on what the clamped rows duplicate)"""
    R.set_compute_dtype(dt)
    B, N = 2, 128
    Lp = 16 * -(-Lr // 16)
    xp, yp = (5.0 * randn(B, Lp, P, N, seed=20)).to(dt).to(DEV), (3.0 * randn(B, Lp, P, N, seed=21)).to(dt).to(DEV)
    full = fused(xp, yp, dt, form)
    got = fused(xp[:, :Lr].contiguous(), yp[:, :Lr].contiguous(), dt, form)
    assert torch.isfinite(got[..., :DOUT]).all()
    assert torch.equal(got, full[:, :Lr, :Lr])


# ------------------------------------------------------------------------------------------------ nothing else is written
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("B,N,Lr", [(2, 128, 17), (2, 64, 9)], ids=lambda v: str(v))
def test_nothing_outside_the_output_is_written(B, N, Lr, dt):
    R.set_compute_dtype(dt)
    x, y, _, _ = case(B, N, Lr, dt)
    xt, yt = operands(x, y, dt)
    G = 64 * LD   # guard elements before and behind (a multiple of 16 bytes in both types): more than a whole tile row
    n = B * Lr * Lr * DOUT
    buf = torch.full((G + n + G,), -7.0, device=DEV, dtype=torch.float32)
    out = fused(xt, yt, dt, "out", out=buf[G:G + n].view(B, Lr, Lr, DOUT))
    assert (buf[:G] == -7.0).all() and (buf[G + n:] == -7.0).all()
    assert torch.equal(out, fused(xt, yt, dt, "out"))   # every element of the block was written
    n = B * Lr * Lr * LD
    buf = torch.full((G + n + G,), 3.0, device=DEV, dtype=dt)
    feat = fused(xt, yt, dt, "y", out=buf[G:G + n].view(B, Lr, Lr, LD))
    assert (buf[:G] == 3.0).all() and (buf[G + n:] == 3.0).all()
    assert (feat[..., DOUT:] == 3.0).all()
    assert torch.equal(feat, fused(xt, yt, dt, "y"))


# ------------------------------------------------------------------------------------------------ nothing outside the operands is used
@pytest.mark.parametrize("form", ["out", "y"])
@pytest.mark.parametrize("B,N,Lr", [(2, 128, 17), (2, 64, 9), (1, 128, 1)], ids=lambda v: str(v))
def test_nothing_outside_the_operands_is_read(B, N, Lr, form):
    dt = torch.bfloat16
    x, y, _, _ = case(B, N, Lr, dt)
    xt, yt = operands(x, y, dt)
    Np = xt.shape[-1]
    G, n = 16 * P * Np, B * Lr * P * Np   # sixteen residues of NaN on either side: a whole tile of rows

    def embedded(t):
        buf = torch.full((G + n + G,), float("nan"), device=DEV, dtype=dt)
        v = buf[G:G + n].view(B, Lr, P, Np)
        v.copy_(t)
        return v
    got = fused(embedded(xt), embedded(yt), dt, form)
    assert torch.isfinite(got).all()
    assert torch.equal(got, fused(xt, yt, dt, form))


# ------------------------------------------------------------------------------------------------ rectangles
@functools.lru_cache(maxsize=None)
def square40(dt):
    x, y, _, _ = case(2, 128, 40, dt)
    xt, yt = operands(x, y, dt)
    return xt, yt, fused(xt, yt, dt, "out"), fused(xt, yt, dt, "y")


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("r0,r1", [(5, 22), (7, 8), (24, 40)])
def test_a_block_of_rows_equals_those_rows_of_the_square(r0, r1, dt):
    R.set_compute_dtype(dt)
    xt, yt, sq_out, sq_y = square40(dt)
    xr = xt[:, r0:r1].contiguous()
    out = fused(xr, yt, dt, "out")
    assert out.shape == (2, r1 - r0, 40, DOUT) and torch.equal(out, sq_out[:, r0:r1])
    assert torch.equal(fused(xr, yt, dt, "y"), sq_y[:, r0:r1])
    # and a block of columns: the transposed rectangle (a column tail with whole row tiles)
    yc = yt[:, r0:r1].contiguous()
    assert torch.equal(fused(xt, yc, dt, "out"), sq_out[:, :, r0:r1])


def test_run_rows_takes_the_fused_route():
    dt = torch.bfloat16
    R.set_compute_dtype(dt)
    xt, yt, sq_out, _ = square40(dt)
    torch.manual_seed(3)
    mod = R.OuterProductMean(P, DOUT).to(DEV)
    xr = xt[:, 5:22].contiguous()
    with torch.no_grad(), count_fused() as c:
        got = mod.run_rows(xr, yt, xt.shape[-1])
        whole = mod.run(xt, yt, xt.shape[-1])
    assert c.n == 2 and got.shape == (2, 17, 40, DOUT)
    assert torch.equal(got, whole[:, 5:22])
    RT.fused_outer = False
    with torch.no_grad(), count_fused() as c:
        general = mod.run_rows(xr, yt, xt.shape[-1])
    RT.fused_outer = True
    assert c.n == 0
    close(got, general, TOL_OUT, "run_rows fused vs general")


# ------------------------------------------------------------------------------------------------ the modules
MODULE_TOL = {torch.bfloat16: 4e-2, torch.float16: 6e-3}   # tests/test_modules_gpu.py MODES: max |a - b| / max |b|


def state(mod, prefix="m"):
    return {prefix + "." + k: v.detach().float().cpu() for k, v in mod.state_dict().items()}


@functools.lru_cache(maxsize=None)
def module_case():
    """B = 2, N = 100, L = 50: modules (fp32 weights), inputs and the CPU oracle's results, shared by the two modes"""
    B, N, Lr, DM, H = 2, 100, 50, 96, 4
    torch.manual_seed(11)
    opm = R.OuterProductMean(P, DOUT)
    pum = R.PairUpdateWithMsa(d_msa=DM, d_proj=P, d_pair=DOUT, n_heads=H, p_dropout=0.0)
    xa, xb = randn(B, N, Lr, P), randn(B, N, Lr, P, seed=1)
    msa, pair = randn(B, N, Lr, DM), randn(B, Lr, Lr, DOUT)
    att = torch.rand(B, Lr, Lr, H, generator=torch.Generator().manual_seed(5))
    return (opm, pum, xa, xb, msa, pair, att, O.outer_product_mean(state(opm), "m", xa, xb),
            O.pair_update_with_msa(state(pum), "m", msa, pair, att))


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_modules_against_the_oracle(dt):
    R.set_compute_dtype(dt)
    opm, pum, xa, xb, msa, pair, att, ref_o, ref_p = module_case()
    opm, pum = opm.to(DEV), pum.to(DEV)
    with count_fused() as c:
        got = opm(xa.to(DEV), xb.to(DEV))
    assert c.n == 1
    e = max_err(got, ref_o)
    print(f"OuterProductMean: max-norm {e:.3e} tol {MODULE_TOL[dt]:.1e}")
    assert e < MODULE_TOL[dt]
    with count_fused() as c:
        got = pum(msa.to(DEV), pair.to(DEV), att.to(DEV))
    assert c.n == 1
    e = max_err(got, ref_p)
    print(f"PairUpdateWithMsa: max-norm {e:.3e} tol {MODULE_TOL[dt]:.1e}")
    assert e < MODULE_TOL[dt]


GRAD_CEIL = {torch.float16: 1e-2, torch.bfloat16: 5e-2}   # tests/test_outer_backward_gpu.py CEIL


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_backward_records_through_the_fused_route(dt):
    R.set_compute_dtype(dt)
    B, N, Lr = 1, 20, 24
    torch.manual_seed(P + Lr)
    cpu_mod = R.OuterProductMean(P, DOUT)
    g = torch.Generator().manual_seed(Lr)
    with torch.no_grad():   # non-trivial affines and biases (the defaults 1 / 0 would hide their gradients' mistakes)
        for name, p in cpu_mod.named_parameters():
            if p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1 + (1.0 if name == "to_out.0.weight" else 0.0))
    x = torch.randn(B, N, Lr, P, generator=g).to(dt).float()
    y = (0.1 * torch.randn(B, N, Lr, P, generator=g)).to(dt).float()
    w = torch.randn(B, Lr, Lr, DOUT, generator=g)
    # float64 autograd through the oracle, from the operands as the mode holds them
    Pd = {k: v.double().requires_grad_() for k, v in state(cpu_mod).items()}
    xd, yd = x.double().requires_grad_(), y.double().requires_grad_()
    (O.outer_product_mean(Pd, "m", xd, yd) * w.double()).sum().backward()
    mod = R.OuterProductMean(P, DOUT)
    mod.load_state_dict(cpu_mod.state_dict())
    mod = mod.to(DEV).enable_backward()
    assert mod.fused_ok(P, N, Lr)
    xg, yg = x.to(DEV).requires_grad_(), y.to(DEV).requires_grad_()
    with count_fused() as c:
        out = mod(xg, yg)
    assert c.n == 1 and out.requires_grad
    (out * w.to(DEV)).sum().backward()
    assert xg.grad.shape == x.shape and yg.grad.shape == y.shape
    for key, got, ref in [("x", xg.grad, xd.grad), ("y", yg.grad, yd.grad)] + \
            [("m." + n_, p.grad, Pd["m." + n_].grad) for n_, p in mod.named_parameters()]:
        e = l2_err(got, ref)
        print(f"{key}: err {e:.3e} ceiling {GRAD_CEIL[dt]:.1e}")
        assert got.shape == ref.shape and e < GRAD_CEIL[dt], (key, e)


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("form", ["out", "y"])
def test_two_runs_give_the_same_bits(form):
    dt = torch.bfloat16
    x, y, _, _ = case(2, 128, 33, dt)
    xt, yt = operands(x, y, dt)
    assert torch.equal(fused(xt, yt, dt, form), fused(xt, yt, dt, form))
