"""GPU parity tests of the librfmi kernels against plain fp32 PyTorch formulas of the same op.
bf16 tolerances: operands are rounded to bf16 (rel 2^-8), accumulation is fp32."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from rosettafold_pytorch_amd import ops, _lib as L  # noqa: E402

DEV = "cuda"


def rel_err(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-20)).item()


def randn(*s, dtype=torch.float32, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(s))
    return torch.randn(*s, generator=g).to(DEV).to(dtype)


@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 2e-2), (torch.float32, 2e-5)])
@pytest.mark.parametrize("M,N,K", [(20000, 288, 288), (20000, 1152, 288), (17000, 384, 768), (16500, 256, 512),
                                   (256, 128, 64), (300, 288, 288), (1024, 384, 384), (130, 37, 96), (64, 80, 128),
                                   (257, 1152, 288), (96, 288, 1152), (512, 96, 736)])
def test_linear(dtype, tol, M, N, K):
    x, w, b = randn(M, K, dtype=dtype), randn(N, K, dtype=dtype, seed=1), randn(N, seed=2)
    ref = x.float() @ w.float().t() + b
    for out_dtype in (torch.float32, dtype):
        y = ops.linear(x, w, b, out_dtype=out_dtype)
        assert rel_err(y, ref) < tol, (M, N, K, out_dtype)
    res = randn(M, N, seed=3)
    y = ops.linear(x, w, b, out_dtype=torch.float32, act=L.ACT_RELU, residual=res)
    assert rel_err(y, torch.relu(ref) + res) < tol


@pytest.mark.parametrize("M,N,K", [(16384, 256, 288), (16384, 1536, 288), (32768, 288, 512), (16384, 288, 1152),
                                   (16384, 384, 768), (16384, 1152, 384), (16384, 128, 64), (16384, 384, 72),
                                   (65536 + 256, 512, 96), (16384, 2304, 384), (16384, 576, 128), (16384, 256, 112),
                                   (16384, 192, 176)])
def test_gemm_persistent_fast_path(M, N, K):
    """Plain row-major panels with M % 256 == 0 take the persistent kernel (gemm_fast.hip): every output type /
    bias / ReLU / residual specialisation, K tails of 8..56, more tiles than CUs and fewer."""
    x, w, b = randn(M, K, dtype=torch.bfloat16), randn(N, K, dtype=torch.bfloat16, seed=1), randn(N, seed=2)
    ref = x.float() @ w.float().t()
    y = ops.linear(x, w, None, out_dtype=torch.bfloat16)
    assert rel_err(y, ref) < 2e-2
    y = ops.linear(x, w, b, out_dtype=torch.bfloat16, act=L.ACT_RELU)
    assert rel_err(y, torch.relu(ref + b)) < 2e-2
    y = ops.linear(x, w, b, out_dtype=torch.float32)
    assert rel_err(y, ref + b) < 2e-2
    res = randn(M, N, seed=3)
    y = ops.linear(x, w, b, out_dtype=torch.float32, residual=res)
    assert rel_err(y, ref + b + res) < 2e-2
    # the generic kernel (explicit tile) must agree with it to fp32 rounding on the same bf16 operands
    y2 = ops.linear(x, w, b, out_dtype=torch.float32, residual=res, tile_cfg=13 if N % 256 == 0 else 1)
    assert rel_err(y, y2) < 1e-5


@pytest.mark.parametrize("M,N,K", [(16384, 256, 288), (16384 + 192, 1536, 288), (16384, 1152, 288), (32768, 384, 288),
                                   (16384, 256, 384), (16384 + 64, 2304, 384), (16384, 1152, 384), (16384, 128 * 5, 384)])
def test_gemm_wreg_skinny_k(M, N, K):
    """K = 288 / 384 projections take the register-resident-weights kernel (gemm_wreg.hip): exact on small integers (any
    row / column / K-slot / swizzle mix-up shows up exactly), bias + ReLU, random data vs fp32, ragged row-tile counts."""
    from rosettafold_pytorch_amd._lib import lib
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-3, 4, (M, K), generator=g).to(DEV).bfloat16()
    w = torch.randint(-3, 4, (N, K), generator=g).to(DEV).bfloat16()
    b = torch.randint(-4, 5, (N,), generator=g).to(DEV).float()
    y = ops.linear(x, w, None, out_dtype=torch.bfloat16)
    assert lib.rf_gemm_last_family() == 4
    ref = x.float() @ w.float().t()
    assert torch.equal(y.float(), ref.bfloat16().float())
    y = ops.linear(x, w, b, out_dtype=torch.bfloat16, act=L.ACT_RELU)
    assert torch.equal(y.float(), torch.relu(ref + b).bfloat16().float())
    xr, wr = randn(M, K, dtype=torch.bfloat16), randn(N, K, dtype=torch.bfloat16, seed=1)
    y = ops.linear(xr, wr, b, out_dtype=torch.bfloat16)
    assert rel_err(y, xr.float() @ wr.float().t() + b) < 2e-2
    y2 = ops.linear(xr, wr, b, out_dtype=torch.bfloat16, tile_cfg=1)  # generic kernel on the same operands
    assert lib.rf_gemm_last_family() == 1
    assert rel_err(y, y2.float()) < 1e-2


@pytest.mark.parametrize("K", [288, 384])
def test_gemm_wreg_split_c(K):
    """The head-major (split-C) output of the skinny-K kernel: [rows/L, G, L, 32] from plain operands, exact."""
    from rosettafold_pytorch_amd._lib import lib
    Lr, dh, N = 128, 32, 1152
    rows_bn, G = 128, N // dh
    M = rows_bn * Lr
    g = torch.Generator().manual_seed(6)
    x = torch.randint(-3, 4, (M, K), generator=g).to(DEV).bfloat16()
    w = torch.randint(-3, 4, (N, K), generator=g).to(DEV).bfloat16()
    b = torch.randint(-2, 3, (N,), generator=g).to(DEV).float()
    out = torch.full((rows_bn, G, Lr, dh), 7.0, device=DEV, dtype=torch.bfloat16)
    ops.gemm(x, w, out, M, N, K, bias=b, c_row=(Lr, G * Lr * dh, dh), c_col=(dh, Lr * dh))
    assert lib.rf_gemm_last_family() == 4
    ref = (x.float() @ w.float().t() + b).view(rows_bn, Lr, G, dh).permute(0, 2, 1, 3)
    assert torch.equal(out.float(), ref.bfloat16().float())


def test_gemm_persistent_exact_integers():
    """Small-integer operands: any row / column / K-chunk mix-up of the persistent kernel shows up exactly."""
    M, N, K = 16384, 288, 136
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randint(-3, 4, (M, K), generator=g).to(DEV).bfloat16()
    w = torch.randint(-3, 4, (N, K), generator=g).to(DEV).bfloat16()
    for od in (torch.float32, torch.bfloat16):
        y = ops.linear(x, w, None, out_dtype=od)
        assert torch.equal(y.float(), x.float() @ w.float().t())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("N,K", [(288, 512), (288, 288), (288, 1152), (384, 384), (384, 768), (384, 1536)])
def test_gemm_persistent_fused_layernorm(N, K, dt):
    """Residual GEMM over whole-row tiles (288-wide pair rows: 256 x 288 tiles; 384-wide MSA rows: 128 x 384 tiles): the
    persistent kernel adds the residual, writes the fp32 rows and emits LayerNorm_next(rows) in the 16-bit type from the same
    epilogue (no second launch) -- the form the forward uses (ops.linear_residual_ln), in both 16-bit builds."""
    import torch.nn as nn
    import rosettafold_pytorch_amd as R
    R.set_compute_dtype(dt)
    try:
        M = 32768
        x, w, b = randn(M, K, dtype=dt), randn(N, K, dtype=dt, seed=1) * 0.1, randn(N, seed=2)
        res = randn(M, N, seed=3) * 2 + 0.5
        res[:7] += 40.0  # rows whose mean dwarfs their spread: the single-pass variance must survive it
        lnm = nn.LayerNorm(N).to(DEV)
        with torch.no_grad():
            lnm.weight.copy_(randn(N, seed=4)); lnm.bias.copy_(randn(N, seed=5))
        ref = res + x.float() @ w.float().t() + b
        ref_ln = torch.nn.functional.layer_norm(ref, (N,), lnm.weight, lnm.bias, lnm.eps)
        out = res.clone()
        assert ops.FUSE_LN
        xn = ops.linear_residual_ln(x, w, b, out, lnm)
        assert L.lib.rf_gemm_last_family() == 3  # the persistent kernel took it
        assert xn is not None and xn.dtype == dt
        tol = 1.0 if dt == torch.bfloat16 else 0.15
        assert rel_err(out, ref) < 2e-2 * tol
        assert rel_err(xn, ref_ln) < 3e-2 * tol
        # against the two-launch form on the same operands: identical fp32 rows, LayerNorm equal to 16-bit rounding
        out2 = res.clone()
        ops.linear(x, w, b, out=out2, residual=out2)
        assert torch.equal(out, out2) or rel_err(out, out2) < 1e-6
        xn2 = ops.layernorm(out2, lnm.weight.detach(), lnm.bias.detach(), eps=lnm.eps, out_dtype=dt)
        assert rel_err(xn, xn2) < 1e-2 * tol
        # twice: bitwise equal
        out3 = res.clone()
        xn3 = ops.linear_residual_ln(x, w, b, out3, lnm)
        assert torch.equal(out3, out) and torch.equal(xn3, xn)
    finally:
        R.set_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,with_ln", [(384, True), (384, False), (288, True), (288, False)])
def test_ffn_fused(D, with_ln, dt):
    """rf_ffn_fused (csrc/ffn.hip, opt-in RF_FUSED_FFN=1): x_res += W2 relu(W1 xn + b1) + b2 [+ the next LayerNorm] in one
    launch, hidden activations on chip, against an fp32 formula with the same 16-bit rounding of the hidden activations and
    against the two-GEMM path; several tiles per workgroup (M = 128 * 3 * CUs would be slow: 40960 rows = 320 tiles)."""
    import torch.nn as nn
    import rosettafold_pytorch_amd as R
    R.set_compute_dtype(dt)
    old = ops.FUSE_FFN
    try:
        torch.manual_seed(D + with_ln)
        M = 40960
        ff = R.FeedForward(D, 4 * D, 0.0).to(DEV)
        lnm = nn.LayerNorm(D).to(DEV)
        with torch.no_grad():
            lnm.weight.copy_(randn(D, seed=4)); lnm.bias.copy_(randn(D, seed=5))
        xn, x0 = randn(M, D, dtype=dt), randn(M, D, seed=3) * 2 + 0.5
        x0[:7] += 40.0

        def run(fused):
            ops.FUSE_FFN = fused
            x = x0.clone()
            return x, ff.apply_residual(xn, x, lnm if with_ln else None)
        xa, la = run(True)
        assert ops.ffn_fused_applies(xn, x0, D, 4 * D)
        xb, lb = run(False)
        w1, w2 = ff.net[0].weight.to(dt).float(), ff.net[3].weight.to(dt).float()
        hid = torch.relu(xn.float() @ w1.t() + ff.net[0].bias).to(dt).float()
        ref = x0 + hid @ w2.t() + ff.net[3].bias
        tol = 1.0 if dt == torch.bfloat16 else 0.15
        assert rel_err(xa, ref) < 1e-3 * tol + 2e-5          # fp32 accumulation of 16-bit products: summation order only
        assert rel_err(xa, xb) < 2e-5
        if with_ln:
            ref_ln = torch.nn.functional.layer_norm(ref, (D,), lnm.weight, lnm.bias, lnm.eps)
            assert la is not None and la.dtype == dt and rel_err(la, ref_ln) < 3e-2 * tol
            assert rel_err(la, lb) < 1e-2 * tol
        else:
            assert la is None
        xc, lc = run(True)                                     # twice: bitwise equal
        assert torch.equal(xa, xc) and (la is None or torch.equal(la, lc))
    finally:
        ops.FUSE_FFN = old
        R.set_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("cfg", list(range(1, 19)))
def test_gemm_all_tile_configs(cfg):
    M, N, K = 777, 600, 352
    x, w = randn(M, K, dtype=torch.bfloat16), randn(N, K, dtype=torch.bfloat16, seed=1)
    y = ops.linear(x, w, None, out_dtype=torch.float32, tile_cfg=cfg)
    assert rel_err(y, x.float() @ w.float().t()) < 1e-2


@pytest.mark.parametrize("N,K", [(288, 512), (288, 1152), (384, 768), (96, 64)])
def test_gemm_fused_residual_layernorm(N, K):
    """C = residual + x W^T + b with the NEXT LayerNorm fused into the epilogue (bf16 path)."""
    import torch.nn as nn
    M = 1000
    x, w, b = randn(M, K, dtype=torch.bfloat16), randn(N, K, dtype=torch.bfloat16, seed=1) * 0.1, randn(N, seed=2)
    res = randn(M, N, seed=3) * 2 + 0.5
    lnm = nn.LayerNorm(N).to(DEV)
    with torch.no_grad():
        lnm.weight.copy_(randn(N, seed=4)); lnm.bias.copy_(randn(N, seed=5))
    ref = res + x.float() @ w.float().t() + b
    ref_ln = torch.nn.functional.layer_norm(ref, (N,), lnm.weight, lnm.bias, lnm.eps)
    out = res.clone()
    ops.FUSE_LN_ANY = True
    try:
        xn = ops.linear_residual_ln(x, w, b, out, lnm)
    finally:
        ops.FUSE_LN_ANY = False
    assert xn is not None and xn.dtype == torch.bfloat16
    assert rel_err(out, ref) < 2e-2
    assert rel_err(xn, ref_ln) < 3e-2


def test_gemm_exact_integers_layout():
    """A = small integers, asymmetric B: any row/col swap or k permutation shows up exactly."""
    M, N, K = 128, 96, 64
    a = (torch.arange(M * K).reshape(M, K) % 7 - 3).float()
    b = ((torch.arange(N * K).reshape(N, K) * 3 + torch.arange(N)[:, None]) % 5 - 2).float()
    y = ops.linear(a.to(DEV).bfloat16(), b.to(DEV).bfloat16(), None, out_dtype=torch.float32)
    assert torch.equal(y.cpu(), a @ b.t())


@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 2e-2), (torch.float32, 2e-5)])
def test_gemm_batched_chunked(dtype, tol):
    """tied-attention logits: logits[b,h,i,j] = sum_{n,d} q[b,n,i,h,d] k[b,n,j,h,d]  (rf.py:254)."""
    B, N, Lr, H, dh = 2, 5, 40, 3, 8
    D = H * dh
    qk = randn(B, N, Lr, 2 * D, dtype=dtype)
    q, k = qk[..., :D].float().view(B, N, Lr, H, dh), qk[..., D:].float().view(B, N, Lr, H, dh)
    ref = torch.einsum("bnihd,bnjhd->bhij", q, k)
    out = torch.empty(B, H, Lr, Lr, device=DEV, dtype=torch.float32)
    ops.gemm(qk, qk, out, Lr, Lr, N * dh, batch=(B, H, 1), b_off=D,
             a_bs=(N * Lr * 2 * D, dh, 0), a_row=(0, 0, 2 * D), a_ko=Lr * 2 * D,
             b_bs=(N * Lr * 2 * D, dh, 0), b_row=(0, 0, 2 * D), b_ko=Lr * 2 * D, kc=dh,
             c_bs=(H * Lr * Lr, Lr * Lr, 0), c_row=(0, 0, Lr))
    assert rel_err(out, ref) < tol


@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 2e-2), (torch.float32, 2e-5)])
def test_gemm_split_rows_cols(dtype, tol):
    """att @ v with v stored transposed [b,n,(h,d),l] and the output scattered to [b,n,l,(h,d)] (rf.py:257-258)."""
    B, N, Lr, H, dh = 2, 3, 24, 2, 8
    D = H * dh
    att = randn(B, H, Lr, Lr, dtype=dtype)
    v_t = randn(B, N, D, Lr, dtype=dtype, seed=5)
    ref = torch.einsum("bhij,bnhdj->bnihd", att.float(), v_t.float().view(B, N, H, dh, Lr)).reshape(B, N, Lr, D)
    out = torch.empty(B, N, Lr, D, device=DEV, dtype=dtype)
    ops.gemm(att, v_t, out, Lr, N * dh, Lr, batch=(B, H, 1),
             a_bs=(H * Lr * Lr, Lr * Lr, 0), a_row=(0, 0, Lr),
             b_bs=(N * D * Lr, dh * Lr, 0), b_row=(dh, D * Lr, Lr),
             c_bs=(N * Lr * D, dh, 0), c_row=(0, 0, D), c_col=(dh, Lr * D))
    assert rel_err(out, ref) < tol


@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 2e-2), (torch.float32, 3e-5)])
@pytest.mark.parametrize("dil", [1, 2, 4])
def test_conv3x3(dtype, tol, dil):
    B, Hh, Ww, Cc, Co = 2, 19, 19, 24, 40
    x = randn(B, Hh, Ww, Cc, dtype=dtype)
    w = randn(Co, Cc, 3, 3, dtype=dtype, seed=1)
    ref = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), w.float(), padding="same", dilation=dil)
    wk = w.permute(0, 2, 3, 1).reshape(Co, 9 * Cc).contiguous()
    out = torch.empty(B, Hh, Ww, Co, device=DEV, dtype=torch.float32)
    ops.gemm(x, wk, out, B * Hh * Ww, Co, 9 * Cc, conv=(B, Hh, Ww, Cc, dil))
    assert rel_err(out, ref.permute(0, 2, 3, 1)) < tol


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("dil,Hh,Ww,bias", [(1, 12, 256, False), (2, 9, 256, True), (4, 20, 256, False), (8, 18, 512, True)])
def test_conv3x3_c288_halo_kernel(dil, Hh, Ww, bias, dt):
    """csrc/conv288.hip (the ResNet pair refiner's 288 -> 288 channel convolutions on rows of whole 256-pixel tiles: the
    three column taps of a row tap read one haloed LDS image) against conv2d, and bit for bit against the generic
    implicit-GEMM kernel (same MFMA products, same fp32 accumulation order per output up to the tap order)."""
    import rosettafold_pytorch_amd as R
    R.set_compute_dtype(dt)
    try:
        B, C = 2, 288
        x = (randn(B, Hh, Ww, C) * 0.5).to(dt)
        w = (randn(C, C, 3, 3, seed=1) * 0.05).to(dt)
        b = randn(C, seed=2) if bias else None
        ref = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), w.float(), b, padding="same", dilation=dil).permute(0, 2, 3, 1)
        wk = w.permute(0, 2, 3, 1).reshape(C, 9 * C).contiguous()
        out = torch.empty(B, Hh, Ww, C, device=DEV, dtype=dt)
        ops.gemm(x, wk, out, B * Hh * Ww, C, 9 * C, conv=(B, Hh, Ww, C, dil), bias=b)
        assert L.lib.rf_gemm_last_family() == 2
        tol = 1.0 if dt == torch.bfloat16 else 0.15
        assert rel_err(out, ref) < 1.2e-2 * tol
        out2 = torch.empty_like(out)          # tile_cfg pins the generic kernel (256 x 288 x 64 tiles)
        ops.gemm(x, wk, out2, B * Hh * Ww, C, 9 * C, conv=(B, Hh, Ww, C, dil), bias=b, tile_cfg=14)
        assert rel_err(out, out2) < 1e-2 * tol   # both round the same fp32 sums (in a different order) to 16 bits
    finally:
        R.set_compute_dtype(torch.bfloat16)


def test_relu_eps_epilogue():
    M, N, K = 70, 288, 64
    x, w = randn(M, K, dtype=torch.bfloat16), randn(N, K, dtype=torch.bfloat16, seed=1)
    y = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    ops.gemm(x, w, y, M, N, K, act=L.ACT_RELU_EPS, act_nvalid=266, act_eps=1e-3)
    ref = torch.relu(x.float() @ w.float().t()) + 1e-3
    ref[:, 266:] = 0
    assert rel_err(y, ref) < 2e-2 and (y[:, 266:] == 0).all()
    ops.gemm(w, x, (yt := torch.empty(N, M, device=DEV, dtype=torch.bfloat16)), N, M, K, act=L.ACT_RELU_EPS,
             act_nvalid=-266, act_eps=1e-3)
    assert rel_err(yt, ref.t()) < 2e-2 and (yt[266:] == 0).all()


@pytest.mark.parametrize("D", [32, 72, 288, 384, 1024, 2304])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_layernorm(D, dtype):
    x = randn(37, D) * 3 + 1
    g, b = randn(D, seed=1), randn(D, seed=2)
    ref = torch.nn.functional.layer_norm(x, (D,), g, b)
    y = ops.layernorm(x, g, b, out_dtype=dtype)
    assert rel_err(y, ref) < (1e-2 if dtype == torch.bfloat16 else 1e-5)


@pytest.mark.parametrize("D,rows", [(1024, 1000), (768, 333), (1024, 20000)])
@pytest.mark.parametrize("odt", [torch.bfloat16, torch.float32])
def test_layernorm_wide_bf16_rows(D, rows, odt):
    """bf16 rows of 513..1024 (the outer-product LayerNorm, rf.py:416) take the 16-byte vectorised kernel."""
    x = (randn(rows, D) * 3 + 1).bfloat16()
    g, b = randn(D, seed=1), randn(D, seed=2)
    ref = torch.nn.functional.layer_norm(x.float(), (D,), g, b)
    y = ops.layernorm(x, g, b, out_dtype=odt)
    assert rel_err(y, ref) < (1e-2 if odt == torch.bfloat16 else 1e-5)


@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("odt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("rows", [5, 1001, 70000])
def test_layernorm_narrow_rows(D, odt, rows):
    """fp32 rows of 32 / 64 values: several rows per wave instruction; plus the grouped affine + LeakyReLU form of the
    SE(3) radial MLPs (ea/modules.py:265-275)."""
    x = randn(rows, D) * 3 + 1
    g, b = randn(D, seed=1), randn(D, seed=2)
    ref = torch.nn.functional.layer_norm(x, (D,), g, b)
    y = ops.layernorm(x, g, b, out_dtype=odt)
    assert rel_err(y, ref) < (1e-2 if odt == torch.bfloat16 else 1e-5)
    if odt == torch.float32 and rows >= 8:
        G = 8
        gg, bb = randn(G, D, seed=3), randn(G, D, seed=4)
        idx = torch.arange(rows, device=DEV) % G
        ref = torch.nn.functional.leaky_relu(torch.nn.functional.layer_norm(x, (D,)) * gg[idx] + bb[idx], 0.01)
        y = ops.layernorm(x, gg, bb, out_dtype=odt, groups=G, act=L.ACT_LEAKY)
        assert rel_err(y, ref) < 1e-5


@pytest.mark.parametrize("B,H,N,Lr", [(1, 2, 5, 64), (2, 3, 37, 128), (1, 12, 16, 192), (2, 12, 128, 256)])
def test_tied_logits_softmax(B, H, N, Lr):
    """One-launch tied-attention logits + softmax (csrc/tied.hip) against the einsum/softmax formula (rf.py:254-265) on
    the same bf16 operands laid out as the q|k|p projection output [B,N,L,3D]."""
    dh = 32
    D = H * dh
    qkp = (randn(B, N, Lr, 3 * D) * (0.6 / math.sqrt(N))).bfloat16()
    q = qkp[..., :D].float().view(B, N, Lr, H, dh)
    k = qkp[..., D:2 * D].float().view(B, N, Lr, H, dh)
    ref = torch.einsum("bnihd,bnjhd->bhij", q, k).softmax(-1)
    att = torch.empty(B, H, Lr, Lr, device=DEV, dtype=torch.bfloat16)
    sym = torch.empty(B, Lr, Lr, H, device=DEV, dtype=torch.float32)
    ops.tied_logits_softmax(qkp, qkp[..., D:], N * Lr * 3 * D, Lr * 3 * D, 3 * D, att, sym, B, H, N, Lr, dh)
    assert rel_err(att, ref) < 1.5e-2
    assert (att.float().sum(-1) - 1).abs().max() < 2e-2
    a = att.float()
    assert rel_err(sym, (0.5 * (a + a.transpose(-1, -2))).permute(0, 2, 3, 1)) < 1e-6
    assert torch.equal(sym, sym.transpose(1, 2))  # reference tests/test_module.py:406-413


@pytest.mark.parametrize("B,H,N,Lr,weights", [(1, 2, 16, 64, True), (2, 3, 48, 128, True), (1, 12, 16, 192, False),
                                              (2, 12, 128, 256, True), (1, 12, 128, 256, False), (1, 2, 64, 256, True),
                                              (1, 2, 256, 256, True), (1, 3, 24, 256, False), (1, 2, 12, 256, True)])
def test_tied_attention_head_major(B, H, N, Lr, weights):
    """The tied-attention core of the bench path (csrc/tied.hip): logits (+ in-kernel position weights) + softmax, the
    symmetrised map and attention.V on head-major operands [B,N,3H,L,32], against the einsum formulas of rf.py:252-265
    evaluated in fp32 on the same bf16 operands."""
    dh = 32
    D = H * dh
    qkv = (randn(B, N, 3 * H, Lr, dh) * (0.9 / math.sqrt(math.sqrt(N)))).bfloat16()
    q, k, v = qkv[:, :, :H], qkv[:, :, H:2 * H], qkv[:, :, 2 * H:]
    w = torch.rand(B, H, N, Lr, device=DEV).softmax(2).contiguous() if weights else None
    qs = 0.37
    qf = q.float()
    if weights:
        qf = (qf * (w.permute(0, 2, 1, 3).unsqueeze(-1) * qs)).bfloat16().float()  # the kernel rounds q*w to bf16 (as the reference's bf16 run would)
    ref_att = torch.einsum("bnhid,bnhjd->bhij", qf, k.float()).softmax(-1)
    att = torch.empty(B, H, Lr, Lr, device=DEV, dtype=torch.bfloat16)
    sym = torch.empty(B, Lr, Lr, H, device=DEV, dtype=torch.float32)
    out = torch.empty(B, N, Lr, D, device=DEV, dtype=torch.bfloat16)
    ops.tied_attention(q, k, v, out.view(B, N, Lr, H, dh).permute(0, 1, 3, 2, 4), att, w=w, qscale=qs if weights else 1.0, att_sym=sym)
    assert rel_err(att, ref_att) < 1.5e-2
    if Lr == 256 and not (weights and N > 192):  # (the one-pass kernel's weight tile stops at N = 192)
        # L = 256 runs contraction-split by default (partial logits + softmax kernel); the one-pass kernel must agree
        att1 = torch.empty_like(att)
        ops.tied_attention(q, k, v, torch.empty_like(out).view(B, N, Lr, H, dh).permute(0, 1, 3, 2, 4), att1, w=w,
                           qscale=qs if weights else 1.0, partial_ws=False)
        assert rel_err(att1, ref_att) < 1.5e-2 and rel_err(att, att1) < 8e-3
    a = att.float()
    assert rel_err(sym, (0.5 * (a + a.transpose(-1, -2))).permute(0, 2, 3, 1)) < 1e-6
    ref_out = torch.einsum("bhij,bnhjd->bnihd", a, v.float()).reshape(B, N, Lr, D)  # A.V on the bf16 probabilities the kernel wrote
    assert rel_err(out, ref_out) < 1e-2
    # exact-integer check of the A.V indexing (row / column / key-order mix-ups show up exactly)
    g = torch.Generator().manual_seed(3)
    att_i = torch.randint(0, 3, (B, H, Lr, Lr), generator=g).to(DEV).bfloat16()
    v_i = torch.randint(-2, 3, (B, N, H, Lr, dh), generator=g).to(DEV).bfloat16()
    out_i = torch.empty(B, N, H, Lr, dh, device=DEV, dtype=torch.bfloat16)
    from rosettafold_pytorch_amd._lib import lib, I64x4
    import ctypes as C
    vs = I64x4(*v_i.stride()[:4])
    rc = lib.rf_tied_av(ops.ptr(att_i), ops.ptr(v_i), C.byref(vs), ops.ptr(out_i), C.byref(vs), B, H, N, Lr, dh, ops.stream())
    assert rc == 0
    ref_i = torch.einsum("bhij,bnhjd->bnhid", att_i.float(), v_i.float())
    assert torch.equal(out_i.float(), ref_i.bfloat16().float())


def test_tied_row_attention_functional_and_custom_op():
    B, N, Lr, H, dh = 1, 16, 64, 4, 32
    q, k, v = (randn(B, N, Lr, H, dh, seed=s_) * 0.4 for s_ in (0, 1, 2))
    q, k, v = q.bfloat16(), k.bfloat16(), v.bfloat16()
    att = torch.einsum("bnihd,bnjhd->bhij", q.float(), k.float()).softmax(-1)
    ref = torch.einsum("bhij,bnjhd->bnihd", att, v.float()).reshape(B, N, Lr, H * dh)
    out, sym = ops.tied_row_attention(q, k, v)
    assert rel_err(out, ref) < 2e-2 and rel_err(sym, (0.5 * (att + att.transpose(-1, -2))).permute(0, 2, 3, 1)) < 1.5e-2
    import rosettafold_pytorch_amd.custom_ops  # noqa: F401  (registers torch.ops.rfmi.*)
    out2, sym2 = torch.ops.rfmi.tied_row_attention(q, k, v)
    assert torch.equal(out2, out) and torch.equal(sym2, sym)


@pytest.mark.parametrize("B,N,Lr,D,H", [(2, 16, 8, 96, 12), (1, 128, 64, 384, 12), (2, 48, 20, 64, 1)])
def test_poswise_collapsed(B, N, Lr, D, H):
    """w[b,h,n,l] = softmax_n(scale * xn[b,n,l,:] . u[b,l,h,:]) on the matrix pipe vs the fp32 formula (rf.py:205-217)."""
    xn = randn(B, N, Lr, D).bfloat16()
    u = (randn(B, Lr, H, D, seed=1) * 0.3).bfloat16()
    w = ops.poswise_collapsed(xn, u, 0.25)
    ref = (torch.einsum("bnlc,blhc->bhnl", xn.float(), u.float()) * 0.25).softmax(2)
    assert rel_err(w, ref) < 1e-4
    assert (w.sum(2) - 1).abs().max() < 1e-5  # reference tests/test_module.py:180-200


@pytest.mark.parametrize("N,BNexp", [(1152, 288), (768, 256), (576, 192), (384, 128)])
def test_gemm_persistent_split_c(N, BNexp):
    """Persistent GEMM with the split-C (head-major) epilogue: out[(b n), g, l, 32] from plain [M, K] x [N, K] operands;
    exact on small integers, and equal to the generic kernel's split addressing."""
    Lr, dh, K = 128, 32, 96
    rows_bn, G = 128, N // dh
    M = rows_bn * Lr
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-3, 4, (M, K), generator=g).to(DEV).bfloat16()
    w = torch.randint(-3, 4, (N, K), generator=g).to(DEV).bfloat16()
    b = torch.randint(-2, 3, (N,), generator=g).to(DEV).float()
    out = torch.full((rows_bn, G, Lr, dh), 7.0, device=DEV, dtype=torch.bfloat16)
    ops.gemm(x, w, out, M, N, K, bias=b, c_row=(Lr, G * Lr * dh, dh), c_col=(dh, Lr * dh))
    ref = (x.float() @ w.float().t() + b).view(rows_bn, Lr, G, dh).permute(0, 2, 1, 3)
    assert torch.equal(out.float(), ref.bfloat16().float())
    out2 = torch.empty_like(out)
    ops.gemm(x, w, out2, M, N, K, bias=b, c_row=(Lr, G * Lr * dh, dh), c_col=(dh, Lr * dh), tile_cfg=1)  # generic kernel
    assert torch.equal(out, out2)


@pytest.mark.parametrize("B,N,Lr", [(1, 128, 16), (2, 128, 48), (1, 64, 32)],
                         ids=["1-128-16-column-split", "2-128-48-column-split", "1-64-32-column-split"])
def test_outer_product_fused(B, N, Lr):
    """Fused OuterProductMean (csrc/outer.hip): outer product over the MSA depth -> LayerNorm(1024) -> Linear(1024 -> 288) in
    one kernel, against einsum + layer_norm + linear in fp32 on the same bf16 inputs (rf.py:412-427)."""
    P, Dout = 32, 288
    x, y = randn(B, N, Lr, P).bfloat16(), (randn(B, N, Lr, P, seed=1) * 0.3).bfloat16()
    g_, b_ = 1.0 + 0.2 * randn(P * P, seed=2), 0.1 * randn(P * P, seed=3)
    w, bias = randn(Dout, P * P, seed=4) * 0.05, randn(Dout, seed=5)
    co = torch.einsum("bniu,bnjv->bijuv", x.float(), y.float()).reshape(B, Lr, Lr, P * P)
    ref = torch.nn.functional.linear(torch.nn.functional.layer_norm(co, (P * P,), g_, b_, 1e-5), w, bias)
    out = ops.outer_product_ln_linear(x, y, g_, b_, w, bias, 1e-5)
    assert rel_err(out, ref) < 1.5e-2
    # exact structure check: with gamma = 1, beta = 0 and a W that picks single features the kernel must reproduce LN(co)[k]
    sel = torch.zeros(Dout, P * P, device=DEV)
    ks = torch.randperm(P * P, generator=torch.Generator().manual_seed(7))[:Dout].to(DEV)
    sel[torch.arange(Dout, device=DEV), ks] = 1.0
    out = ops.outer_product_ln_linear(x, y, torch.ones(P * P, device=DEV), torch.zeros(P * P, device=DEV), sel,
                                      torch.zeros(Dout, device=DEV), 1e-5)
    ref = torch.nn.functional.layer_norm(co, (P * P,))[..., ks]
    assert rel_err(out, ref) < 1.5e-2  # (bf16 rounding of the raw blocks; an index mix-up would be O(1))
    # with the consumer's LayerNorm(288) in the epilogue (bf16 rows written into a wider feature tensor)
    g2, b2 = 1.0 + 0.2 * randn(Dout, seed=8), 0.1 * randn(Dout, seed=9)
    xt = x.permute(0, 2, 3, 1).contiguous()
    yt = y.permute(0, 2, 3, 1).contiguous()
    wp, s_, c_ = ops.outer_fold(w, g_, b_, bias)
    feat = torch.full((B, Lr, Lr, 304), 3.0, device=DEV, dtype=torch.bfloat16)
    ops.outer_fused(xt, yt, wp, s_, c_, None, 1e-5, ln2=(g2, b2, 1e-5, feat, 304))
    ref1 = torch.nn.functional.linear(torch.nn.functional.layer_norm(co, (P * P,), g_, b_, 1e-5), w, bias)
    assert rel_err(feat[..., :Dout], torch.nn.functional.layer_norm(ref1, (Dout,), g2, b2, 1e-5)) < 2e-2
    assert (feat[..., Dout:] == 3.0).all()
    import rosettafold_pytorch_amd.custom_ops  # noqa: F401
    out2 = torch.ops.rfmi.outer_product_ln_linear(x, y, g_, b_, w, bias, 1e-5)
    assert rel_err(out2, torch.nn.functional.linear(torch.nn.functional.layer_norm(co, (P * P,), g_, b_, 1e-5), w, bias)) < 1.5e-2


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("offset", [0.0, 1.0, 4.0])
def test_outer_product_fused_offset_mean(offset, dt):
    """the fused kernel contracts the 16-bit-rounded RAW outer-product block with W' and removes the block mean
    algebraically afterwards, so its error scales with |mu| / sigma of the block (the two-launch form normalises in fp32
    first).  Stated bound, asserted: relative L2 <= c (1 + 0.6 |mu|/sigma), c = 3e-3 (bf16) / 3.75e-4 (fp16); observed at
    |mu|/sigma = 0 / 7.7 / 32: 2.0e-3 / 1.2e-2 / 4.9e-2 (bf16), 2.5e-4 / 1.5e-3 / 6.1e-3 (fp16).  Trained proj_msa LayerNorms with a
    large beta are the case to run in the fp16 mode (tools/outer_offset_mean.py sweeps the ratio)."""
    import rosettafold_pytorch_amd as R
    R.set_compute_dtype(dt)
    try:
        B, N, Lr, P, Dout = 1, 64, 64, 32, 288
        x, y = (randn(B, N, Lr, P) + offset).to(dt), (randn(B, N, Lr, P, seed=1) * 0.3 + offset).to(dt)
        g_, b_ = 1.0 + 0.2 * randn(P * P, seed=2), 0.1 * randn(P * P, seed=3)
        w, bias = randn(Dout, P * P, seed=4) * 0.05, randn(Dout, seed=5)
        co = torch.einsum("bniu,bnjv->bijuv", x.float(), y.float()).reshape(B, Lr, Lr, P * P)
        ratio = (co.mean(-1).abs() / co.std(-1)).median().item()
        ref = torch.nn.functional.linear(torch.nn.functional.layer_norm(co, (P * P,), g_, b_, 1e-5), w, bias)
        out = ops.outer_product_ln_linear(x, y, g_, b_, w, bias, 1e-5)
        e2 = ((out - ref).norm() / ref.norm()).item()
        c = 3e-3 if dt == torch.bfloat16 else 3.75e-4
        assert e2 < c * (1 + 0.6 * ratio), (offset, ratio, e2)
    finally:
        R.set_compute_dtype(torch.bfloat16)


def test_gemm_block_layernorm_epilogue():
    """Outer-product GEMM with LayerNorm(1024) of every 32x32 output block in the epilogue (OuterProductMean, rf.py:416,
    424-426) against einsum + layer_norm; operands / output laid out exactly as the model's call."""
    B, Lr, P, N = 2, 24, 32, 72
    PP = P * P
    x_t, y_t = randn(B, Lr, P, N, dtype=torch.bfloat16), randn(B, Lr, P, N, dtype=torch.bfloat16, seed=1)
    g, b = randn(PP, seed=2), randn(PP, seed=3)
    co = torch.empty(B, Lr, Lr, PP, device=DEV, dtype=torch.bfloat16)
    ops.gemm(x_t, y_t, co, Lr * P, Lr * P, N, batch=(B, 1, 1), a_bs=(Lr * P * N, 0, 0), b_bs=(Lr * P * N, 0, 0),
             c_bs=(Lr * Lr * PP, 0, 0), c_row=(P, Lr * PP, P), c_col=(P, PP), act=L.ACT_BLOCK_LN32, block_ln=(g, b, 1e-5))
    outer = torch.einsum("biun,bjvn->bijuv", x_t.float(), y_t.float()).reshape(B, Lr, Lr, PP)
    ref = torch.nn.functional.layer_norm(outer, (PP,), g, b, 1e-5)
    assert rel_err(co, ref) < 1.5e-2


@pytest.mark.parametrize("n", [4 * 1000 + 4, 1001, 1 << 20])
def test_axpby(n):
    """y = a x + b z: vectorised (n % 4 == 0) and scalar paths, mixed dtypes, in place."""
    x, z = randn(n), randn(n, seed=1)
    y = ops.axpby(x, 0.5, z, 0.25, torch.empty(n, device=DEV, dtype=torch.float32))
    assert rel_err(y, 0.5 * x + 0.25 * z) < 1e-6
    yb = ops.axpby(x, 0.5, z.bfloat16(), 0.25, torch.empty(n, device=DEV, dtype=torch.bfloat16))
    assert rel_err(yb, 0.5 * x + 0.25 * z.bfloat16().float()) < 1e-2
    x2 = x.clone()
    ops.axpby(x2, 1.0, z, 1.0, x2)
    assert rel_err(x2, x + z) < 1e-6
    ys = ops.axpby(x, 2.0, None, 0.0, torch.empty(n, device=DEV, dtype=torch.float32))
    assert rel_err(ys, 2.0 * x) < 1e-6


@pytest.mark.parametrize("D,Lr", [(288, 24), (384, 10), (96, 12)])
def test_sym_layernorm(D, Lr):
    """LayerNorm (no affine) of the symmetrised pair tensor 0.5 * (x + x^T) in one pass (rf.py:550-566)."""
    x = randn(2, Lr, Lr, D) * 2 + 0.3
    ref = torch.nn.functional.layer_norm(0.5 * (x + x.transpose(1, 2)), (D,))
    assert rel_err(ops.sym_layernorm(x, torch.float32), ref) < 1e-5
    assert rel_err(ops.sym_layernorm(x, torch.bfloat16), ref) < 1e-2


def test_tile_1d_feats():
    """feat[b,i,j,c0 + c] = m[b,i,c], feat[b,i,j,c0 + P2 + c] = m[b,j,c] (rf.py:476-485), vectorised path."""
    B, Lr, P2, Kf, c0 = 2, 9, 64, 200, 32
    m1 = randn(B, Lr, P2)
    for dt in (torch.bfloat16, torch.float32):
        feat = torch.zeros(B, Lr, Lr, Kf, device=DEV, dtype=dt)
        ops.tile_1d_feats(m1, feat, Kf, c0, B, Lr, P2)
        ref = torch.zeros(B, Lr, Lr, Kf, device=DEV)
        ref[..., c0:c0 + P2] = m1[:, :, None, :]
        ref[..., c0 + P2:c0 + 2 * P2] = m1[:, None, :, :]
        assert rel_err(feat, ref) < (1e-2 if dt == torch.bfloat16 else 1e-7)
        assert (feat[..., :c0] == 0).all() and (feat[..., c0 + 2 * P2:] == 0).all()


def test_softmax_and_tied():
    B, H, Lr = 2, 3, 50
    lg = randn(B, H, Lr, Lr) * 4
    att = torch.empty(B, H, Lr, Lr, device=DEV, dtype=torch.float32)
    sym = torch.empty(B, Lr, Lr, H, device=DEV, dtype=torch.float32)
    ops.tied_softmax(lg, att, sym, H)
    ref = lg.softmax(-1)
    assert rel_err(att, ref) < 1e-5
    assert rel_err(sym, (0.5 * (ref + ref.transpose(-1, -2))).permute(0, 2, 3, 1)) < 1e-5
    assert torch.equal(sym, sym.transpose(1, 2))  # reference tests/test_module.py:406-413


@pytest.mark.parametrize("xdt", [torch.float32, torch.bfloat16])
def test_instnorm(xdt):
    B, Hh, Cc = 2, 37, 72
    x = (randn(B, Hh, Hh, Cc) * 2 + 0.5).to(xdt).float()
    g, b, r = randn(Cc, seed=1), randn(Cc, seed=2), randn(B, Hh, Hh, Cc, seed=3)
    ref = torch.nn.functional.instance_norm(x.permute(0, 3, 1, 2), weight=g, bias=b, eps=1e-6).permute(0, 2, 3, 1)
    y, y2 = ops.instnorm(x.to(xdt), g, b, residual=r, act=L.ACT_ELU, out_dtype=torch.float32, out2_dtype=torch.bfloat16)
    assert rel_err(y, torch.nn.functional.elu(ref + r)) < 1e-5
    assert rel_err(y2, y) < 1e-2
