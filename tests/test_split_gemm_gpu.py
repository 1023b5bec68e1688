"""rf_gemm with the split-bf16 fp32 operand code RF_F32X3 (the "high" float32 matmul precision) against a float64 product of
the same operands: every addressing form and epilogue of the exact fp32 kernel, odd M / N / K edges, both libraries.

Bound per element (include/rfmi.h): |C - C64| <= (3 * 2^-16 + K * 2^-23) * (|A| |B|^T) * |alpha| + fp32 rounding of the
bias / residual / activation.  The rounding of lo and the dropped lo.lo product are each at most 2^-16 |a b|."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import _lib as L  # noqa: E402
from rosettafold_pytorch_amd import ops  # noqa: E402

import gemm_oracle as O  # noqa: E402

DEV = "cuda"


@pytest.fixture(autouse=True)
def high_f32():
    R.set_compute_dtype(torch.float32)
    R.set_float32_matmul_precision("high")
    yield
    R.set_float32_matmul_precision("highest")
    R.set_compute_dtype(torch.bfloat16)


def rnd(*s, seed=0):
    return torch.randn(*s, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float()


def run(A, B, C, *a, exact=False, **kw):
    """one rf_gemm on fresh copies of C; returns (C, kernel family)"""
    C = C.clone()
    ops.gemm(A, B, C, *a, exact=exact, **kw)
    fam = L.lib.rf_gemm_last_family()
    torch.cuda.synchronize()
    return C, fam


def check_bound(got, Ae, Be, K, **kw):
    """the shared per-element check (tests/gemm_oracle.py) with this kernel's operand-precision term"""
    return O.check_bound(got, Ae, Be, K, op_term=3 * 2.0 ** -16 + K * 2.0 ** -23, **kw)


# ------------------------------------------------------------------------------------------------ plain / batched
@pytest.mark.parametrize("M,N,K", [(133, 77, 45), (257, 130, 96), (64, 64, 32), (1, 5, 3), (515, 291, 288), (300, 96, 21),
                                   (70, 200, 1030)])
def test_plain(M, N, K):
    A, B = rnd(M, K, seed=1).to(DEV), rnd(N, K, seed=2).to(DEV)
    C, fam = run(A, B, torch.zeros(M, N, device=DEV), M, N, K)
    assert fam == 5
    check_bound(C, A, B, K)


def test_batched_with_broadcast():
    M, N, K = 37, 45, 40
    A = rnd(2, 3, M, K, seed=3).to(DEV)
    B = rnd(2, 1, N, K, seed=4).to(DEV)  # broadcast over the middle batch dimension (b_bs[1] = 0)
    C, fam = run(A, B, torch.zeros(2, 3, M, N, device=DEV), M, N, K, batch=(2, 3, 1), a_bs=(3 * M * K, M * K, 0),
                 b_bs=(N * K, 0, 0), c_bs=(3 * M * N, M * N, 0))
    assert fam == 5
    check_bound(C, A, B.expand(2, 3, N, K), K)


def test_split_rows_and_k_chunks():
    # A rows in groups of rc = 5 with padding rows between groups; K in chunks of kc with a gap between chunks (both sides)
    G, rc, K = 7, 5, 48
    for kc, gap in ((12, 3), (8, 4)):  # element-wise staging / 16-byte staging
        nch = K // kc
        Ast = rnd(G, rc + 2, nch, kc + gap, seed=5).to(DEV)
        Bst = rnd(19, nch, kc + gap, seed=6).to(DEV)
        M, N = G * rc, 19
        C, fam = run(Ast, Bst, torch.zeros(M, N, device=DEV), M, N, K, kc=kc,
                     a_row=(rc, (rc + 2) * nch * (kc + gap), nch * (kc + gap)), a_ko=kc + gap,
                     b_row=(0, 0, nch * (kc + gap)), b_ko=kc + gap)
        assert fam == 5
        Ae = Ast[:, :rc, :, :kc].reshape(M, K)
        Be = Bst[:, :, :kc].reshape(N, K)
        check_bound(C, Ae, Be, K)


def test_split_output_rows_and_columns():
    M, N, K, cc = 50, 48, 24, 16
    A, B = rnd(M, K, seed=7).to(DEV), rnd(N, K, seed=8).to(DEV)
    # C stored as [N / cc][M / 10][10 + 2][cc]: row groups of 10 with 2 padding rows, column groups of cc
    Cst = torch.zeros(N // cc, M // 10, 12, cc, device=DEV)
    C, fam = run(A, B, Cst, M, N, K, c_row=(10, 12 * cc, cc), c_col=(cc, (M // 10) * 12 * cc))
    assert fam == 5
    got = C[:, :, :10, :].permute(1, 2, 0, 3).reshape(M, N)
    check_bound(got, A, B, K)
    assert (C[:, :, 10:, :] == 0).all()


@pytest.mark.parametrize("c", [16, 6])  # 16-byte staging / element-wise staging
def test_conv3x3(c):
    n, h, w, co, dil = 2, 9, 11, 21, 2
    x = rnd(n, h, w, c, seed=9).to(DEV)
    W = rnd(co, 9, c, seed=10).to(DEV)
    M, K = n * h * w, 9 * c
    C, fam = run(x, W, torch.zeros(M, co, device=DEV), M, co, K, conv=(n, h, w, c, dil))
    assert fam == 5
    # effective im2col operand: Ae[pixel, tap * c + ch]
    xp = F.pad(x.permute(0, 3, 1, 2), (dil, dil, dil, dil))
    cols = []
    for t in range(9):
        di, dj = (t // 3) * dil, (t % 3) * dil
        cols.append(xp[:, :, di:di + h, dj:dj + w].permute(0, 2, 3, 1).reshape(M, c))
    Ae = torch.cat(cols, 1)
    check_bound(C, Ae, W.reshape(co, K), K)
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), W.view(co, 3, 3, c).permute(0, 3, 1, 2).double(), padding=dil, dilation=dil)
    assert torch.allclose(C.view(n, h, w, co).permute(0, 3, 1, 2).double(), ref, rtol=0, atol=1e-3)


# ------------------------------------------------------------------------------------------------ epilogues
EPI = [
    dict(bias_mode=L.BIAS_COL, act=L.ACT_NONE),
    dict(bias_mode=L.BIAS_ROW, act=L.ACT_RELU),
    dict(bias_mode=L.BIAS_COL, act=L.ACT_ELU, alpha=0.37),
    dict(bias_mode=None, act=L.ACT_RELU_EPS, nvalid=29, eps=1e-3),
    dict(bias_mode=L.BIAS_COL, act=L.ACT_RELU_EPS, nvalid=-40, eps=1e-3, residual=True),
    dict(bias_mode=L.BIAS_ROW, act=L.ACT_NONE, alpha=-1.5, residual=True),
]


@pytest.mark.parametrize("e", EPI, ids=[f"epi{i}" for i in range(len(EPI))])
@pytest.mark.parametrize("MNK", [(96, 64, 64), (77, 53, 45)])  # 4-wide and element-wise stores
def test_epilogue(e, MNK):
    M, N, K = MNK
    A, B = rnd(M, K, seed=11).to(DEV), rnd(N, K, seed=12).to(DEV)
    bias = None
    if e["bias_mode"] is not None:
        bias = rnd(N if e["bias_mode"] == L.BIAS_COL else M, seed=13).to(DEV)
    res = rnd(M, N, seed=14).to(DEV) if e.get("residual") else None
    kw = dict(bias=bias, bias_mode=e["bias_mode"], act=e["act"], act_nvalid=e.get("nvalid", 0), act_eps=e.get("eps", 0.0),
              alpha=e.get("alpha", 1.0), residual=res)
    C, fam = run(A, B, torch.zeros(M, N, device=DEV), M, N, K, **kw)
    assert fam == 5
    check_bound(C, A, B, K, alpha=kw["alpha"], bias=bias, bias_mode=e["bias_mode"], res=res, act=e["act"],
                nvalid=kw["act_nvalid"], eps=kw["act_eps"])
    # in place: C = residual + ...
    if res is not None:
        Cin = res.clone()
        ops.gemm(A, B, Cin, M, N, K, **{**kw, "residual": Cin})
        torch.cuda.synchronize()
        assert torch.equal(Cin, C)


def test_16bit_output():
    M, N, K = 130, 72, 64
    A, B = rnd(M, K, seed=15).to(DEV), rnd(N, K, seed=16).to(DEV)
    C, fam = run(A, B, torch.zeros(M, N, device=DEV, dtype=torch.bfloat16), M, N, K, bias=rnd(N, seed=17).to(DEV))
    assert fam == 5
    check_bound(C.float(), A, B, K, bias=rnd(N, seed=17), c16=True)


# ------------------------------------------------------------------------------------------------ properties
def test_much_more_accurate_than_bf16():
    M, N, K = 256, 288, 384
    A, B = rnd(M, K, seed=18).to(DEV), rnd(N, K, seed=19).to(DEV)
    ref = A.double() @ B.double().T
    C3, _ = run(A, B, torch.zeros(M, N, device=DEV), M, N, K)
    R.set_compute_dtype(torch.bfloat16)
    Cb = torch.zeros(M, N, device=DEV)
    ops.gemm(A.bfloat16(), B.bfloat16(), Cb, M, N, K)
    torch.cuda.synchronize()
    R.set_compute_dtype(torch.float32)
    rms3 = (C3.double() - ref).pow(2).mean().sqrt().item()
    rmsb = (Cb.double() - ref).pow(2).mean().sqrt().item()
    print(f"\n[split gemm] rms error split {rms3:.3e}, bf16 {rmsb:.3e}, ratio {rmsb / rms3:.0f}")
    assert rms3 * 50 <= rmsb, (rms3, rmsb)


def test_routing_and_exact_pin():
    M, N, K = 64, 64, 32
    A, B = rnd(M, K, seed=20).to(DEV), rnd(N, K, seed=21).to(DEV)
    _, fam = run(A, B, torch.zeros(M, N, device=DEV), M, N, K)
    assert fam == 5
    _, fam = run(A, B, torch.zeros(M, N, device=DEV), M, N, K, exact=True)
    assert fam == 0
    R.set_float32_matmul_precision("highest")
    _, fam = run(A, B, torch.zeros(M, N, device=DEV), M, N, K)
    assert fam == 0


def test_bitwise_reproducible():
    M, N, K = 515, 291, 288
    A, B = rnd(M, K, seed=22).to(DEV), rnd(N, K, seed=23).to(DEV)
    C1, _ = run(A, B, torch.zeros(M, N, device=DEV), M, N, K)
    C2, _ = run(A, B, torch.zeros(M, N, device=DEV), M, N, K)
    assert torch.equal(C1, C2)


def test_both_libraries_identical():
    cases = [((257, 130, 96), {}), ((77, 53, 45), {"alpha": 0.5})]
    for (M, N, K), kw in cases:
        A, B = rnd(M, K, seed=24).to(DEV), rnd(N, K, seed=25).to(DEV)
        out = []
        for code in (L.RF_BF16, L.RF_F16):
            L.select_h16(code)
            C, fam = run(A, B, torch.zeros(M, N, device=DEV), M, N, K, **kw)
            assert fam == 5
            out.append(C)
        L.select_h16(L.RF_BF16)
        assert torch.equal(out[0], out[1])


def test_nonfinite_positions_match_exact():
    M, N, K = 40, 36, 24
    A, B = rnd(M, K, seed=26), rnd(N, K, seed=27)
    A[3, 5] = math.inf
    A[10, 1] = -math.inf
    B[7, 2] = math.nan
    A[20, :] = 0.0
    A[20, 4] = math.inf  # inf times the exact zeros / bf16-exact values of B
    B[9, 4] = 0.0
    B[11, 4] = 1.0
    A, B = A.to(DEV), B.to(DEV)
    C3, _ = run(A, B, torch.zeros(M, N, device=DEV), M, N, K)
    Ce, _ = run(A, B, torch.zeros(M, N, device=DEV), M, N, K, exact=True)
    assert torch.equal(torch.isfinite(C3), torch.isfinite(Ce))
    assert torch.equal(torch.isnan(Ce) & torch.isnan(C3), torch.isnan(Ce))  # a NaN of the exact product is a NaN here too
    fin = torch.isfinite(Ce)
    assert (C3[fin] - Ce[fin]).abs().max().item() < 1e-3


def _rc(fn):
    try:
        fn()
    except L.RfmiError as e:
        return str(e)
    return None


def test_rejects_what_the_exact_path_rejects():
    M, N, K = 256, 256, 64
    A, B = rnd(M, K, seed=28).to(DEV), rnd(N, K, seed=29).to(DEV)
    C = torch.zeros(M, N, device=DEV)
    g, b = torch.ones(1024, device=DEV), torch.zeros(1024, device=DEV)
    lnout = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    rs = torch.ones(M, device=DEV)
    bad = [
        dict(act=L.ACT_BLOCK_LN32, block_ln=(g, b, 1e-5)),
        dict(ln=(lnout, g[:N], b[:N], 1e-5)),
        dict(rs=(rs, M, M, 16, 32, 1.0)),
        dict(alpha=0.0), dict(alpha=-0.0), dict(alpha=math.inf), dict(alpha=math.nan),  # a product scaled by zero is a fill
        dict(alpha=0.0, bias=torch.ones(N, device=DEV)),
    ]
    for kw in bad:
        r3 = _rc(lambda: ops.gemm(A, B, C, M, N, K, **kw))
        re = _rc(lambda: ops.gemm(A, B, C, M, N, K, exact=True, **kw))
        assert r3 is not None and r3 == re, (kw.keys(), r3, re)
        assert "RF_EINVAL" in r3
