"""Every rf_gemm kernel family against a float64 product of its effective operands, per output element, driven from the
descriptor (tests/gemm_oracle.py): the generic 16-bit tile kernel at each of its 18 tile shapes, the implicit 3x3 convolution
and the 288-channel halo kernel, the persistent kernel, the register-resident-weights kernel and the exact fp32 kernel, in
both 16-bit libraries; every epilogue, addressing form and alignment fallback of the dispatch at the smallest shape that
reaches it.  Each case also asserts the kernel family that ran, that no element outside C's image was written (sentinels in
every gap and 64 elements around) and -- NaN sits in every operand gap -- that nothing outside the operands was read.

The bound is derived, not measured.  With prod = alpha A B^T, mag = |alpha| |A| |B|^T and x = the float64 result after bias,
activation and residual, for the 16-bit families

    tol = (K + 8) 2^-23 (mag + |bias|) + 2^-22 (|x| + |prod|) + out |x| + tiny

  (K + 8) 2^-23 (mag + |bias|)   fp32 accumulation of the exact 16-bit products -- twice the textbook K 2^-24, because the
                                 summation order inside an MFMA is not documented -- and the generic kernel's fold of
                                 bias / alpha into the accumulators (two roundings of the bias, and it rides the sum);
  2^-22 (|x| + |prod|)           the fp32 roundings of the epilogue: alpha, activation, residual add;
  out |x|                        the rounding of the stored value: 0 for fp32 C, 2^-8 for bfloat16, 2^-11 for fp16;
  tiny                           1e-30; 2^-24 for fp16 C (its subnormal spacing);
  ELU adds 4e-6 |x|              the fast exponential, as in the split-bf16 tests.

and for the exact fp32 kernel  tol = (K + 4) 2^-24 mag + 2^-22 (|x| + |prod|) + out |x|  (a k-ordered fma chain).

The fused-LayerNorm output of the persistent kernel is held to a float64 layer_norm of the float64 rows; its bound is the
propagation of the row bound t = max tol of the row through the normalisation plus the fp32 statistics (ln_tol below).
rf_ffn_fused is two such contractions with the hidden activations rounded to the 16-bit type in between (ffn_tol below).

Worst err / tol seen on an MI355X, per family and output type (bfloat16 library / fp16 library); the same figures on the
kernels before and after the epilogues' maximum was made NaN-propagating, which changes no finite result:
    0 exact fp32                fp32 C 0.134          bfloat16 C 0.987
    1 generic 16-bit            fp32 C 0.035 / 0.047  16-bit C 0.994 / 0.986
    2 conv3x3 and halo          fp32 C 0.007 / 0.010  16-bit C 0.981 / 0.962
    3 persistent                fp32 C 0.015 / 0.016  16-bit C 0.991 / 0.965   fused LayerNorm output 0.992 / 0.974
    4 register-resident weights                       16-bit C 0.969 / 0.832
    rf_ffn_fused                fp32 C 0.098 / 0.043
A 16-bit C sits just under 1 by construction: `out` is the half-ulp of the output type, which round-to-nearest reaches at the
start of a binade; the arithmetic (the fp32 C figures) uses a few per cent of its bound.  (Printed at the end of the module with -s.)

Non-finite operands (test_nonfinite_*): the result is NaN exactly where the float64 reference is NaN (torch.relu keeps NaN),
+-inf with the same sign where it is infinite, finite and inside the bound elsewhere."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import _lib as L  # noqa: E402
from rosettafold_pytorch_amd import ops  # noqa: E402

import gemm_oracle as O  # noqa: E402

DEV = "cuda"
F32 = torch.float32
H16 = [torch.bfloat16, torch.float16]
H16_IDS = ["bf16", "fp16"]

# csrc/gemm.hip: kTiles
TILES = {1: (128, 128, 64), 2: (128, 128, 32), 3: (128, 96, 64), 4: (128, 96, 32), 5: (128, 64, 64), 6: (128, 64, 32),
         7: (64, 128, 64), 8: (64, 128, 32), 9: (64, 96, 64), 10: (64, 96, 32), 11: (64, 64, 64), 12: (64, 64, 32),
         13: (256, 256, 64), 14: (256, 288, 64), 15: (256, 192, 64), 16: (256, 128, 64), 17: (256, 128, 32), 18: (128, 256, 32)}

assert (O.ACT_NONE, O.ACT_RELU, O.ACT_ELU, O.ACT_RELU_EPS) == (L.ACT_NONE, L.ACT_RELU, L.ACT_ELU, L.ACT_RELU_EPS)
assert (O.BIAS_COL, O.BIAS_ROW, O.AMODE_CONV3X3) == (L.BIAS_COL, L.BIAS_ROW, L.AMODE_CONV3X3)

_worst = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for (fam, lib), w in sorted(_worst.items()):
        print(f"\n[gemm bound] family {fam} {lib}: worst err / tol = {w:.4f}", end="")
    print()


@pytest.fixture
def lib(request):
    """the 16-bit library under test (parametrised indirectly with the torch dtype); float32 leaves the bfloat16 one active"""
    dt = request.param
    R.set_compute_dtype(dt)
    try:
        yield dt
    finally:
        R.set_compute_dtype(torch.bfloat16)


def both_libs(fn):
    return pytest.mark.parametrize("lib", H16, ids=H16_IDS, indirect=True)(fn)


def _note(fam, dt, w, cdt=F32):
    key = (f"{fam}, {'fp32' if cdt == F32 else '16-bit'} C", str(dt).replace("torch.", ""))
    _worst[key] = max(_worst.get(key, 0.0), w)


def _vec(n, seed):
    return O._rand(n, seed, DEV)


def run_case(d, dt, cdt, fam, *, A=None, B=None, tile=0, bias_mode=None, bias_shift=0, act=O.ACT_NONE, nvalid=0, eps=0.0,
             alpha=1.0, res=None, res_shift=0, exact=False, nonfinite=False, rs=None, ln=None, what=None):
    """One rf_gemm described by d on operands of dtype dt into C of dtype cdt; asserts the family, the bound and the sentinels.
    A / B: storages to reuse (else fresh ones with NaN in every gap).  res: None | "sep" | "alias" (C = residual + ...).
    bias_shift / res_shift: pointer offsets in elements that break the 16-byte alignment.  Returns (C storage, A, B)."""
    if A is None:
        A = O.make_operand(d, "a", dt, 11, DEV)
    if B is None:
        B = O.make_operand(d, "b", dt, 12, DEV)
    M, N, K = d["M"], d["N"], d["K"]
    bias = None
    if bias_mode is not None:
        bias = _vec((N if bias_mode == O.BIAS_COL else M) + bias_shift, 13)[bias_shift:]
    C0 = O.make_c(d, cdt, device=DEV, extra=res_shift)
    resv = rt = roff = None
    if res == "sep":
        roff = d["c_off"] + res_shift
        rt = O.make_residual(d, 14, res_off=roff, device=DEV)
        resv = O.gather_c(d, rt, roff)
    elif res == "alias":
        assert cdt == F32 and res_shift == 0
        img = (O.c_offsets(d, DEV) + d["c_off"]).reshape(-1)
        C0[img] = _vec(img.numel(), 14)
        resv = O.gather_c(d, C0).clone()
    C = C0.clone()
    kw = O.gemm_kwargs(d)
    if res is not None:
        kw.update(residual=C if res == "alias" else rt, res_off=d["c_off"] if res == "alias" else roff)
    scale = None
    if rs is not None:  # (rs tensor [M / rpb, ncols / cg, rpb], rpb, cg, ncols, rs_alpha)
        t_, rpb, cg, ncols, ra = rs
        kw["rs"] = (t_, t_.shape[1] * rpb, rpb, cg, ncols, ra)
        s = t_.double().permute(0, 2, 1).reshape(M, ncols // cg).repeat_interleave(cg, 1) * ra
        scale = torch.cat([s, torch.ones(M, N - ncols, dtype=torch.float64, device=DEV)], 1)
    if ln is not None:
        kw["ln"] = ln
    ops.gemm(A, B, C, M, N, K, bias=bias, bias_mode=bias_mode, act=act, act_nvalid=nvalid, act_eps=eps, alpha=alpha,
             tile_cfg=tile, exact=exact, **kw)
    got_fam = L.lib.rf_gemm_last_family()
    torch.cuda.synchronize()
    assert got_fam == fam, (got_fam, fam, what)
    if res == "alias":  # outside the image the aliased storage still holds the sentinel
        keep = torch.ones_like(C0, dtype=torch.bool)
        keep[(O.c_offsets(d, DEV) + d["c_off"]).reshape(-1)] = False
        assert torch.equal(C[keep], C0[keep]), what
    else:
        O.assert_untouched(d, C0, C)
    Ae, Be = O.effective_operands(d, A, B)
    h16 = A.dtype != F32
    w = O.check_bound(O.gather_c(d, C).squeeze(0) if Ae.shape[0] == 1 else O.gather_c(d, C),
                      Ae.squeeze(0) if Ae.shape[0] == 1 else Ae, Be.squeeze(0) if Be.shape[0] == 1 else Be, K,
                      op_term=O.op_term_h16(K) if h16 else O.op_term_f32(K), bias_in_acc=h16, alpha=alpha, bias=bias,
                      bias_mode=bias_mode, res=resv.squeeze(0) if resv is not None and Ae.shape[0] == 1 else resv, act=act,
                      nvalid=nvalid, eps=eps, out=O.OUT_ROUND[cdt], tiny=O.OUT_TINY[cdt], nonfinite=nonfinite, scale=scale,
                      what=what)
    _note(fam, dt, w, cdt)
    return C, A, B


# ------------------------------------------------------------------------------------------------ generic kernel: every tile
@both_libs
@pytest.mark.parametrize("tile", list(TILES))
def test_generic_every_tile(tile, lib):
    """two row tiles with the second ragged; a ragged staged (N % 8 == 0) and a scalar (odd N) epilogue; three K steps with the
    last partial and a single partial step with K < BK; fp32 and 16-bit C; a column bias; a three-level batch with B
    broadcast over the middle level"""
    bm, bn, bk = TILES[tile]
    M = bm + 17
    for N in (bn + 24, bn + 21):
        for K in (2 * bk + 24, 8):
            d = O.desc(M, N, K)
            A, B = O.make_operand(d, "a", lib, 1, DEV), O.make_operand(d, "b", lib, 2, DEV)
            for cdt in (F32, lib):
                run_case(d, lib, cdt, 1, A=A, B=B, tile=tile, bias_mode=O.BIAS_COL, what=(tile, N, K, cdt))
    N, K = bn + 24, 2 * bk + 24
    d = O.desc(M, N, K, nb0=2, nb1=3, nb2=1, a_bs=(3 * M * K, M * K, 0), b_bs=(N * K + 8, 0, 0), c_bs=(3 * M * N + 8, M * N, 0))
    run_case(d, lib, F32, 1, tile=tile, bias_mode=O.BIAS_COL, what=(tile, "batch"))
    run_case(d, lib, lib, 1, tile=tile, what=(tile, "batch16"))


# ------------------------------------------------------------------------------------------------ epilogue matrix
EPI_ACTS = [dict(act=O.ACT_NONE), dict(act=O.ACT_RELU), dict(act=O.ACT_ELU), dict(act=O.ACT_RELU_EPS, nvalid=70, eps=1e-3),
            dict(act=O.ACT_RELU_EPS, nvalid=-70, eps=1e-3)]


@both_libs
@pytest.mark.parametrize("N", [104, 100, 101])  # staged / staged for fp32 C only (N % 8 == 4) / scalar for both
@pytest.mark.parametrize("tile", [1, 14, 0])
def test_epilogue_matrix(tile, N, lib):
    M, K = 150, 88
    d = O.desc(M, N, K)
    A, B = O.make_operand(d, "a", lib, 3, DEV), O.make_operand(d, "b", lib, 4, DEV)
    for bias_mode in (None, O.BIAS_COL, O.BIAS_ROW):
        for a in EPI_ACTS:
            for alpha in (1.0, 0.37, -1.5):
                for cdt in (F32, lib):
                    run_case(d, lib, cdt, 1, A=A, B=B, tile=tile, bias_mode=bias_mode, alpha=alpha, what=(bias_mode, a, alpha, cdt), **a)


@both_libs
@pytest.mark.parametrize("N", [104, 100, 101])
@pytest.mark.parametrize("tile", [1, 14, 0])
def test_epilogue_residual_and_misalignment(tile, N, lib):
    """residual into fp32 C (separate and aliasing C) and into 16-bit C; C, bias and residual each one element off their
    16-byte alignment, one at a time (vec_store / stage_epi switch off one cause at a time)"""
    M, K = 150, 88
    d = O.desc(M, N, K)
    A, B = O.make_operand(d, "a", lib, 5, DEV), O.make_operand(d, "b", lib, 6, DEV)
    for a in (dict(act=O.ACT_NONE), dict(act=O.ACT_RELU), dict(act=O.ACT_RELU_EPS, nvalid=-70, eps=1e-3)):
        for alpha in (1.0, -1.5):
            kw = dict(A=A, B=B, tile=tile, bias_mode=O.BIAS_COL, alpha=alpha, **a)
            run_case(d, lib, F32, 1, res="sep", what=("sep", a, alpha), **kw)
            run_case(d, lib, F32, 1, res="alias", what=("alias", a, alpha), **kw)
            run_case(d, lib, lib, 1, res="sep", what=("sep16", a, alpha), **kw)
    d1 = dict(d, c_off=d["c_off"] + 1)
    for cdt in (F32, lib):
        for act in (O.ACT_NONE, O.ACT_ELU):
            kw = dict(A=A, B=B, tile=tile, act=act)
            run_case(d1, lib, cdt, 1, bias_mode=O.BIAS_COL, what=("c+1", cdt, act), **kw)
            run_case(d, lib, cdt, 1, bias_mode=O.BIAS_COL, bias_shift=1, what=("bias+1", cdt, act), **kw)
            run_case(d, lib, cdt, 1, bias_mode=O.BIAS_ROW, bias_shift=1, what=("rowbias+1", cdt, act), **kw)
            run_case(d, lib, cdt, 1, bias_mode=O.BIAS_COL, res="sep", res_shift=1, what=("res+1", cdt, act), **kw)
    run_case(d1, lib, F32, 1, A=A, B=B, tile=tile, bias_mode=O.BIAS_COL, res="sep", what="c+1 and its residual")


# ------------------------------------------------------------------------------------------------ addressing
def _split_c(M, N, rc, cc, pad_rows=2):
    """C stored [N / cc][M / rc][rc + pad_rows][cc] with 8 more elements between column groups"""
    g = (M + rc - 1) // rc
    return dict(c_rc=rc, c_ri=cc, c_ro=(rc + pad_rows) * cc, c_cc=cc, c_co=g * (rc + pad_rows) * cc + 8)


@both_libs
@pytest.mark.parametrize("kc", [0, 8, 16, 40])  # kc = 40 against BK = 64: the chunk cursor crosses two chunks in one step
@pytest.mark.parametrize("tile", [1, 11, 13, 0])
def test_addressing(tile, kc, lib):
    """A and B rows in groups of 5 with 3 padding rows, K = 80 in chunks with 8-element gaps on both operands, operand pointers
    8 elements into their storage, C with split rows and columns (power-of-two and other factors, padding rows between groups)"""
    M, N, K = 160, 48, 80
    nch = K // kc if kc else 1
    ri = nch * ((kc or K) + 8)  # row: nch chunks of kc + 8 elements (the last 8 of each a gap)
    base = dict(kc=kc, a_ko=(kc + 8) if kc else 0, b_ko=(kc + 8) if kc else 0, a_ri=ri, b_ri=ri)
    rows = dict(a_rc=5, a_ro=8 * ri, b_rc=5, b_ro=8 * ri)
    offs = dict(a_off=O.PAD + 8, b_off=O.PAD + 8)
    for extra in (rows, dict(rows, **offs), offs):
        for cs in ({}, _split_c(M, N, 16, 8), _split_c(M, N, 10, 24)):
            d = O.desc(M, N, K, **base, **extra, **cs)
            A, B = O.make_operand(d, "a", lib, 7, DEV), O.make_operand(d, "b", lib, 8, DEV)
            for cdt in (F32, lib):
                run_case(d, lib, cdt, 1, A=A, B=B, tile=tile, bias_mode=O.BIAS_COL, what=(sorted(extra), cs.get("c_rc"), cdt))
    d = O.desc(M, N, K, **base, **rows, **_split_c(M, N, 10, 24))
    run_case(d, lib, F32, 1, tile=tile, bias_mode=O.BIAS_ROW, act=O.ACT_RELU, res="sep", what="split C with residual")


# ------------------------------------------------------------------------------------------------ convolutions
@both_libs
@pytest.mark.parametrize("tile", [1, 11, 13, 14, 0])
def test_conv3x3_generic(tile, lib):
    n, h, w = 2, 5, 7
    for c in (8, 24):
        for co in (21, 40):
            for dil in (1, 2, 4, 8):  # 8 >= h and >= w: only the centre tap is inside the picture
                d = O.desc(n * h * w, co, 9 * c, a_mode=O.AMODE_CONV3X3, conv_n=n, conv_h=h, conv_w=w, conv_c=c, conv_dil=dil,
                           b_ri=9 * c)
                A, B = O.make_operand(d, "a", lib, 9, DEV), O.make_operand(d, "b", lib, 10, DEV)
                for cdt in (F32, lib):
                    for bias_mode in (None, O.BIAS_COL):
                        run_case(d, lib, cdt, 2, A=A, B=B, tile=tile, bias_mode=bias_mode, what=(c, co, dil, cdt, bias_mode))


@both_libs
@pytest.mark.parametrize("H,dil", [(3, 8), (1, 4), (2, 1)])
def test_conv288_halo_kernel(H, dil, lib):
    """the 288-channel halo kernel (csrc/conv288.hip: rows of whole 256-pixel tiles), elementwise against float64"""
    W, c = 256, 288
    d = O.desc(H * W, c, 9 * c, a_mode=O.AMODE_CONV3X3, conv_n=1, conv_h=H, conv_w=W, conv_c=c, conv_dil=dil, b_ri=9 * c)
    A, B = O.make_operand(d, "a", lib, 15, DEV), O.make_operand(d, "b", lib, 16, DEV)
    for bias_mode in (None, O.BIAS_COL):
        run_case(d, lib, lib, 2, A=A, B=B, bias_mode=bias_mode, what=(H, dil, bias_mode))


# ------------------------------------------------------------------------------------------------ persistent kernel
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@both_libs
@pytest.mark.parametrize("M,N,K", [(16384, 128, 64), (16384, 192, 72), (16384 + 256, 288, 136), (16384, 256, 1160),
                                   (16384 + 256, 1024, 64)])
def test_persistent(M, N, K, lib):
    """a_ri = K + 8 with NaN in the gap, c_ri = N + 8 with sentinel columns; (16640, 1024, 64) is 260 tiles of 256 x 256: more
    than the launcher's one workgroup per CU and no multiple of it"""
    if N == 1024:
        nt = (M // 256) * (N // 256)
        assert nt > _cus() and nt % _cus() != 0, (nt, _cus())
    d = O.desc(M, N, K, a_ri=K + 8, b_ri=K + 8, c_ri=N + 8)
    A, B = O.make_operand(d, "a", lib, 17, DEV), O.make_operand(d, "b", lib, 18, DEV)
    kw = dict(A=A, B=B)
    run_case(d, lib, F32, 3, what="f32", **kw)
    run_case(d, lib, F32, 3, bias_mode=O.BIAS_COL, act=O.ACT_RELU, res="sep", what="f32 bias relu res", **kw)
    run_case(d, lib, F32, 3, bias_mode=O.BIAS_COL, res="alias", what="f32 bias res in place", **kw)
    run_case(d, lib, lib, 3, bias_mode=O.BIAS_COL, act=O.ACT_RELU, what="16 bias relu", **kw)
    run_case(d, lib, lib, 3, what="16", **kw)


def ln_tol(x, t, gamma, beta, eps, N, out, tiny):
    """Bound of the fused LayerNorm y = gamma (v - mean) rstd + beta computed in fp32 from rows v with |v - x| <= t (t: the row's
    largest tol), against layer_norm(x) in float64.  With s = rstd, xh = (x - mean) s, u = 2^-24:
      input:       |d(v - mean)| <= 2 t and |d rstd| / rstd <= 2 t s, so |dy| <= |gamma| s 2 t (1 + |xh|);
      statistics:  the fp32 sums of N terms carry N u relative error: the mean is off by N u max|x|, the single-pass variance
                   E[v^2] - mean^2 by (N + 2) u (E[x^2] + mean^2) <= 2 (N + 2) u E[x^2], i.e. rstd by (N + 2) u E[x^2] s^2 relatively,
                   plus 2^-21 for the hardware reciprocal square root;
      output:      out |y| for the 16-bit rounding, 2^-22 (|y| + |beta|) for the fp32 affine."""
    u = 2.0 ** -24
    mean = x.mean(-1, keepdim=True)
    var = x.var(-1, unbiased=False, keepdim=True)
    s = (var + eps).rsqrt()
    xh = (x - mean) * s
    y = xh * gamma + beta
    ex2 = (x * x).mean(-1, keepdim=True)
    stat = (N + 1) * u * x.abs().amax(-1, keepdim=True) + (x - mean).abs() * ((N + 2) * u * ex2 * s * s + 2.0 ** -21)
    return y, gamma.abs() * s * (2 * t * (1 + xh.abs()) + stat) + out * y.abs() + 2.0 ** -22 * (y.abs() + beta.abs()) + tiny


@both_libs
@pytest.mark.parametrize("N,K", [(288, 136), (384, 72)])
def test_persistent_fused_layernorm(N, K, lib):
    M = 16384
    d = O.desc(M, N, K, a_ri=K + 8, c_ri=N)
    A, B = O.make_operand(d, "a", lib, 19, DEV), O.make_operand(d, "b", lib, 20, DEV)
    gamma, beta, eps = _vec(N, 21), _vec(N, 22), 1e-5
    lnout = torch.full((M * N + 2 * O.PAD,), -1234.0, dtype=lib, device=DEV)
    ln0 = lnout.clone()
    C, _, _ = run_case(d, lib, F32, 3, A=A, B=B, bias_mode=O.BIAS_COL, res="alias", ln=(lnout[O.PAD:], gamma, beta, eps))
    # the float64 rows and their bound once more (run_case has asserted C against them)
    Ae, Be = O.effective_operands(d, A, B)
    got = O.gather_c(d, C).squeeze(0)
    bias = _vec(N, 13)
    # (the residual was overwritten in place: rebuild it as run_case did)
    resv = _vec(M * N, 14).view(M, N)
    x, prod, mag, babs = O.reference(Ae.squeeze(0), Be.squeeze(0), bias=bias, res=resv)
    tol = O.op_term_h16(K) * (mag + babs) + 2.0 ** -22 * (x.abs() + prod.abs()) + 1e-30
    assert ((got.double() - x).abs() <= tol).all()
    y, ytol = ln_tol(x, tol.amax(-1, keepdim=True), gamma.double(), beta.double(), eps, N, O.OUT_ROUND[lib], O.OUT_TINY[lib])
    yg = lnout[O.PAD:O.PAD + M * N].view(M, N).double()
    assert torch.isfinite(yg).all()
    w = ((yg - y).abs() / ytol).max().item()
    _note("3 fused LayerNorm", lib, w, lib)
    assert w <= 1.0, w
    assert torch.equal(lnout[:O.PAD], ln0[:O.PAD]) and torch.equal(lnout[O.PAD + M * N:], ln0[O.PAD + M * N:])


# ------------------------------------------------------------------------------------------------ register-resident weights
@both_libs
@pytest.mark.parametrize("M", [16384, 16384 + 64])
@pytest.mark.parametrize("N", [256, 384, 640])  # one per column variant: 256-wide, 384-wide, 128-wide
@pytest.mark.parametrize("K", [288, 384])
def test_wreg(K, N, M, lib):
    d = O.desc(M, N, K, a_ri=K + 8, b_ri=K + 8, c_ri=N + 8)
    A, B = O.make_operand(d, "a", lib, 23, DEV), O.make_operand(d, "b", lib, 24, DEV)
    run_case(d, lib, lib, 4, A=A, B=B, what="plain")
    run_case(d, lib, lib, 4, A=A, B=B, bias_mode=O.BIAS_COL, act=O.ACT_RELU, what="bias relu")


def _head_major(M, N, rc, cc=32):
    """C stored [M / rc][N / cc][rc][cc] (head-major, csrc/tied.hip) with 64 more elements between row groups"""
    return dict(c_rc=rc, c_ri=cc, c_ro=(N // cc) * rc * cc + 64, c_cc=cc, c_co=rc * cc)


@both_libs
@pytest.mark.parametrize("K,N,M,rc", [(288, 256, 16384, 128), (384, 384, 16512, 96), (288, 640, 16512, 96), (384, 256, 16512, 128)])
def test_wreg_split_c(K, N, M, rc, lib):
    """the split-C form; c_rc = 96 is not a power of two (c_rsh == -1: the division)"""
    d = O.desc(M, N, K, a_ri=K + 8, **_head_major(M, N, rc))
    run_case(d, lib, lib, 4, bias_mode=O.BIAS_COL, act=O.ACT_RELU, what=(rc, "bias relu"))
    run_case(d, lib, lib, 4, what=(rc, "plain"))


@both_libs
@pytest.mark.parametrize("K,rc", [(288, 128), (384, 96)])
def test_wreg_row_scale(K, rc, lib):
    """rf_gemm_desc.rs: the leading columns times rs_alpha * rs[row group][column group][row in group], applied to the biased
    accumulator in float64 before the output rounding"""
    N, cg, ncols, ra = 384, 32, 128, 0.25
    M = 16512 if rc == 96 else 16384
    d = O.desc(M, N, K, **_head_major(M, N, rc))
    rs = _vec((M // rc) * (ncols // cg) * rc, 25).view(M // rc, ncols // cg, rc)
    run_case(d, lib, lib, 4, bias_mode=O.BIAS_COL, rs=(rs, rc, cg, ncols, ra), what="rs")


# ------------------------------------------------------------------------------------------------ exact fp32 kernel
@pytest.fixture
def f32_mode():
    R.set_compute_dtype(torch.float32)
    try:
        yield
    finally:
        R.set_compute_dtype(torch.bfloat16)


F32_EPI = [
    dict(bias_mode=O.BIAS_COL, act=O.ACT_NONE),
    dict(bias_mode=O.BIAS_ROW, act=O.ACT_RELU),
    dict(bias_mode=O.BIAS_COL, act=O.ACT_ELU, alpha=0.37),
    dict(bias_mode=None, act=O.ACT_RELU_EPS, nvalid=29, eps=1e-3),
    dict(bias_mode=O.BIAS_COL, act=O.ACT_RELU_EPS, nvalid=-40, eps=1e-3, res="sep"),
    dict(bias_mode=O.BIAS_ROW, act=O.ACT_NONE, alpha=-1.5, res="alias"),
]


@pytest.mark.parametrize("M,N,K", [(133, 77, 45), (257, 130, 96), (64, 64, 32), (1, 5, 3), (515, 291, 288), (300, 96, 21),
                                   (70, 200, 1030)])
def test_exact_f32_plain(M, N, K, f32_mode):
    """the plain shapes of the split-bf16 tests on the exact kernel; K = 21 / 45 / 3 take the element-wise staging (f32_vec == 0),
    and so does an A pointer one element off its alignment"""
    d = O.desc(M, N, K)
    run_case(d, F32, F32, 0, exact=True, what="plain")
    run_case(dict(d, a_off=O.PAD + 1), F32, F32, 0, exact=True, bias_mode=O.BIAS_COL, what="a+1")
    run_case(O.desc(M, N, K, a_ri=K + 4, b_ri=K + 8, c_ri=N + 3), F32, F32, 0, exact=True, what="padded")


@pytest.mark.parametrize("e", F32_EPI, ids=[f"epi{i}" for i in range(len(F32_EPI))])
@pytest.mark.parametrize("MNK", [(96, 64, 64), (77, 53, 45)])  # 4-wide and element-wise stores
def test_exact_f32_epilogue(e, MNK, f32_mode):
    for cdt in (F32, torch.bfloat16):
        if cdt != F32 and e.get("res") == "alias":
            continue
        run_case(O.desc(*MNK), F32, cdt, 0, exact=True, what=cdt, **e)


# ------------------------------------------------------------------------------------------------ non-finite values
def _plant(d, A, B):
    """one NaN, one +inf and one -inf into A, one NaN into B, and a row of A that is exactly zero except for one inf which
    meets one exact 0 and one exact 1 of B"""
    oa, _ = O.operand_offsets(d, "a", DEV)
    ob, _ = O.operand_offsets(d, "b", DEV)
    oa, ob = oa[0] + d["a_off"], ob[0] + d["b_off"]
    A, B = A.clone(), B.clone()
    A[oa[2, 6]] = math.nan
    A[oa[3, 5]] = math.inf
    A[oa[10, 1]] = -math.inf
    B[ob[7, 2]] = math.nan
    A[oa[20]] = 0.0
    A[oa[20, 4]] = math.inf
    B[ob[9, 4]] = 0.0
    B[ob[11, 4]] = 1.0
    return A, B


def _nonfinite(d, dt, cdt, fam, **kw):
    A, B = _plant(d, O.make_operand(d, "a", dt, 27, DEV), O.make_operand(d, "b", dt, 28, DEV))
    for act in (O.ACT_NONE, O.ACT_RELU):
        run_case(d, dt, cdt, fam, A=A, B=B, act=act, nonfinite=True, what=(fam, cdt, act), **kw)
        run_case(d, dt, cdt, fam, A=A, B=B, act=act, bias_mode=O.BIAS_COL, nonfinite=True, what=(fam, cdt, act, "bias"), **kw)


@both_libs
@pytest.mark.parametrize("tile", [0, 1, 14])
def test_nonfinite_generic(tile, lib):
    for N in (104, 101):  # staged and scalar epilogue
        for cdt in (F32, lib):
            _nonfinite(O.desc(150, N, 88), lib, cdt, 1, tile=tile)
    d = O.desc(150, 104, 88)
    A, B = _plant(d, O.make_operand(d, "a", lib, 27, DEV), O.make_operand(d, "b", lib, 28, DEV))
    run_case(d, lib, F32, 1, A=A, B=B, tile=tile, act=O.ACT_RELU_EPS, nvalid=70, eps=1e-3, nonfinite=True, what="relu_eps")


@both_libs
def test_nonfinite_persistent(lib):
    for cdt in (F32, lib):
        _nonfinite(O.desc(16384, 192, 72), lib, cdt, 3)


@both_libs
def test_nonfinite_wreg(lib):
    _nonfinite(O.desc(16384, 256, 288), lib, lib, 4)


def test_nonfinite_exact_f32(f32_mode):
    for MNK in ((96, 64, 64), (77, 53, 45)):
        _nonfinite(O.desc(*MNK), F32, F32, 0, exact=True)


def _plant_both(d, A, B):
    """_plant, and infinities in B as well: one that meets finite values of A only, and one that meets the +inf of A at the
    same k (inf * inf = +inf and inf * -inf = -inf in the exact product: no NaN)"""
    A, B = _plant(d, A, B)
    ob = O.operand_offsets(d, "b", DEV)[0][0] + d["b_off"]
    B[ob[13, 9]] = -math.inf
    B[ob[4, 5]] = math.inf   # A[3, 5] is +inf
    B[ob[5, 5]] = -math.inf
    return A, B


@pytest.mark.parametrize("plant", [_plant, _plant_both], ids=["inf_in_a", "inf_in_both"])
def test_nonfinite_split_bf16(plant, f32_mode):
    """Family 5 to the same statement as the others.  An infinite operand is (hi inf, lo 0); in the cross products it used to meet
    the lo piece of the other operand, which has either sign or is 0, so 86 of the 188 elements whose exact value is +-inf came
    out as NaN (inf - inf, inf * 0).  The cross products now take the hi piece with its non-finite elements zeroed
    (csrc/gemm.hip: bf16x8_finite_or_zero), so inf and NaN enter through hi.hi alone, as through an exact product."""
    R.set_float32_matmul_precision("high")
    try:
        d = O.desc(96, 64, 64)
        A, B = plant(d, O.make_operand(d, "a", F32, 27, DEV), O.make_operand(d, "b", F32, 28, DEV))
        for act in (O.ACT_NONE, O.ACT_RELU):
            C0 = O.make_c(d, F32, device=DEV)
            C = C0.clone()
            ops.gemm(A, B, C, 96, 64, 64, act=act, **O.gemm_kwargs(d))
            assert L.lib.rf_gemm_last_family() == 5
            torch.cuda.synchronize()
            O.assert_untouched(d, C0, C)
            Ae, Be = O.effective_operands(d, A, B)
            got = O.gather_c(d, C)[0]
            x = O.reference(Ae[0], Be[0], act=act)[0]
            gn, xn, xi = torch.isnan(got), torch.isnan(x), torch.isinf(x)
            print(f"\n[gemm bound] split-bf16 act {act}: NaN got {int(gn.sum())} / reference {int(xn.sum())}; NaN at +-inf of the "
                  f"reference {int((gn & xi).sum())} of {int(xi.sum())}, at finite elements {int((gn & ~xn & ~xi).sum())}")
            w = O.check_bound(got, Ae[0], Be[0], 64, op_term=O.op_term_split(64), act=act, nonfinite=True)
            _note(5, F32, w)
    finally:
        R.set_float32_matmul_precision("highest")


def ffn_tol(x, w1, b1, w2, b2, res, r16):
    """rf_ffn_fused: out = res + relu(x W1^T + b1)_16 W2^T + b2.  The hidden pre-activation carries the 16-bit bound t1 (bias in
    the accumulator); ReLU does not enlarge it; its rounding to the 16-bit type adds r16 |h|.  That error passes through |W2|,
    and the second contraction adds its own accumulation term (hidden + 8) 2^-23 (|h| |W2|^T + |b2|) and the fp32 roundings of
    the bias and residual adds."""
    D, hid = x.shape[1], w1.shape[0]
    pre = x @ w1.t() + b1
    t1 = O.op_term_h16(D) * (x.abs() @ w1.abs().t() + b1.abs()) + 2.0 ** -22 * pre.abs()
    h = torch.relu(pre)
    dh = t1 + r16 * h.abs()
    y = h @ w2.t() + b2
    out = res + y
    tol = dh @ w2.abs().t() + O.op_term_h16(hid) * (h.abs() @ w2.abs().t() + b2.abs()) + 2.0 ** -22 * (out.abs() + y.abs() + res.abs()) + 1e-30
    return out, tol


@both_libs
@pytest.mark.parametrize("D", [288, 384])
def test_ffn_fused_bound_and_nonfinite(D, lib):
    """the fused feed-forward against float64, per element; then a NaN and an inf in x: the hidden ReLU keeps the NaN
    (torch.relu does), so the row leaves as NaN"""
    M, hid = 256, 4 * D
    x = _vec(M * D, 31).view(M, D).to(lib)
    w1, w2 = (_vec(hid * D, 32).view(hid, D) * D ** -0.5).to(lib), (_vec(D * hid, 33).view(D, hid) * hid ** -0.5).to(lib)
    b1, b2, res = _vec(hid, 34), _vec(D, 35), _vec(M * D, 36).view(M, D)
    wp = ops.ffn_pack(w1, w2, lib)
    for planted in (False, True):
        xs = x.clone()
        if planted:
            xs[5, 7] = math.nan
            xs[130, 200] = math.inf
        out = res.clone()
        ops.ffn_fused(xs, wp, b1, b2, out)
        torch.cuda.synchronize()
        ref, tol = ffn_tol(xs.double(), w1.double(), b1.double(), w2.double(), b2.double(), res.double(), O.OUT_ROUND[lib])
        rnan, rinf = torch.isnan(ref), torch.isinf(ref)
        assert torch.equal(torch.isnan(out), rnan), (int(torch.isnan(out).sum()), int(rnan.sum()))
        assert torch.equal(out.double()[rinf], ref[rinf])
        if planted:  # (the inf meets both signs in W1, so relu leaves +inf and 0 and W2 makes inf - inf of them)
            assert rnan[5].all() and not torch.isfinite(ref[130]).any() and not rnan[:5].any()
        fin = ~(rnan | rinf)
        assert torch.isfinite(out[fin]).all()
        w = ((out.double() - ref).abs()[fin] / tol[fin]).max().item()
        _note("ffn", lib, w)
        assert w <= 1.0, w


# ------------------------------------------------------------------------------------------------ alpha == 0
def _refused(fn):
    try:
        fn()
    except L.RfmiError as e:
        return str(e)
    return None


@pytest.mark.parametrize("alpha", [0.0, -0.0, math.inf, -math.inf, math.nan])
def test_alpha_zero_or_nonfinite_is_refused(alpha):
    """a product scaled by zero is a fill (and the 16-bit kernels start their accumulators at bias / alpha): RF_EINVAL for
    every operand type, checked through the return code; C is not touched"""
    M, N, K = 64, 64, 32
    bias = torch.ones(N, device=DEV)
    try:
        for dt, mode, exact in ((torch.bfloat16, None, False), (torch.float16, None, False), (F32, "highest", False),
                                (F32, "high", False), (F32, "high", True)):
            R.set_compute_dtype(dt)
            if mode:
                R.set_float32_matmul_precision(mode)
            A, B = torch.ones(M, K, device=DEV, dtype=dt), torch.ones(N, K, device=DEV, dtype=dt)
            for b in (None, bias):
                C = torch.full((M, N), 7.0, device=DEV)
                msg = _refused(lambda: ops.gemm(A, B, C, M, N, K, alpha=alpha, bias=b, exact=exact))
                assert msg is not None and "RF_EINVAL" in msg, (dt, mode, exact, msg)
                assert L.lib.rf_gemm_last_family() == -1
                torch.cuda.synchronize()
                assert (C == 7.0).all()
    finally:
        R.set_float32_matmul_precision("highest")
        R.set_compute_dtype(torch.bfloat16)
