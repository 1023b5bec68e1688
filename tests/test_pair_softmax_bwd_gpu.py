"""rf_pair_softmax_bwd and rf_sym_layernorm_bwd (csrc/backward.hip): the two kernels the backward of MsaUpdateWithPair adds, in
both builds.

Each is held against float64 autograd of a restatement of the forward on the same operands, by the yardstick rule of
tests/grad_oracle.py, with 2^-24, the rounding unit of the fp32 outputs.  A row is one (b, i, z) softmax row of dz, one (b, i, j)
channel row of d pair.

RF_MSA_PAIR_BACKWARD_ERRORS=FILE: the measured errors are also merged into that JSON file (key "kernel_errors")."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import grad_oracle as G  # noqa: E402
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import _lib, ops  # noqa: E402

DEV = "cuda"
# rf_pair_softmax_bwd (B, L, NZ).  L = 1: everything exactly zero; a very short row; two samples of several blocks; either side
# of one wave's 64 lanes with NZ = 12 (a wave takes three maps) and NZ = 5 (odd: the slab's (j, z) split is no power of two,
# one wave takes two maps); a row that crosses 256 threads; and 16 x 1025 x 4 bytes, the first slab past 64 KB of LDS.
SOFTMAX_SHAPES = [(2, 1, 4), (1, 5, 4), (2, 24, 16), (1, 63, 12), (1, 65, 5), (1, 257, 16), (1, 1025, 16)]
# rf_sym_layernorm_bwd (B, L, D, NZ).  L = 1 (the diagonal alone), L = 2, an odd L whose middle row pairs with itself, the
# model's width on one and two 16-byte pieces per lane with 33 and 8 rows; 520 and 1024 channels: four pieces per lane, the
# last with w (64 x 1024 x 4 bytes) read from memory instead of LDS.
SYM_SHAPES = [(2, 1, 32, 4), (1, 2, 32, 8), (2, 5, 72, 12), (1, 33, 288, 16), (1, 8, 288, 4), (1, 3, 520, 4), (1, 3, 1024, 64)]
BUILDS = [("bf16-build", torch.bfloat16), ("f16-build", torch.float16)]
SENTINEL = 7.0
EPS = 1e-5
RECORDS = []
HELD = dict(units=G.UNIT[torch.float32], rows=1, records=RECORDS, key="out")
_restore_mode = G.restore_mode()
_write_records = G.records_fixture("RF_MSA_PAIR_BACKWARD_ERRORS", RECORDS, "max(torch float32 autograd vs float64, 2^-24)")


@pytest.fixture(params=BUILDS, ids=[b[0] for b in BUILDS])
def build(request):
    """both kernels take fp32 operands and are built into both libraries"""
    R.set_compute_dtype(request.param[1])
    return request.param[1]


# ================================================================================================ rf_pair_softmax_bwd
@functools.lru_cache(maxsize=None)
def softmax_case(shape):
    """One set of operands per shape, shared and left unchanged: logits [B,L,L,NZ] normal with a standard deviation of 3, the
    maps' gradient [NZ,B,L,L]."""
    B, L, NZ = shape
    g_ = G.gen(5100 + 7 * L + NZ)
    logits = torch.randn(B, L, L, NZ, generator=g_) * 3
    datt = torch.randn(NZ, B, L, L, generator=g_)
    return dict(logits=logits.to(DEV), datt=datt.to(DEV))


def softmax_autograd(c, dtype):
    """sum(softmax_j(logits[b,i,:,z]) * datt[z,b,i,:]) differentiated by torch; rows [b,i,z,:] so that a row is one softmax"""
    lg = c["logits"].detach().cpu().to(dtype).clone().requires_grad_()
    p = lg.permute(3, 0, 1, 2).softmax(-1)   # [NZ,B,L,L]
    (p * c["datt"].detach().cpu().to(dtype)).sum().backward()
    return lg.grad.permute(0, 1, 3, 2).contiguous()   # [B,L,NZ,L]


@functools.lru_cache(maxsize=None)
def softmax_refs(shape):
    c = softmax_case(shape)
    return softmax_autograd(c, torch.float64), softmax_autograd(c, torch.float32)


def run_softmax_bwd(logits, datt, datt_ld=None, nz_pad=None):
    """the entry point on sentinel-filled outputs with a tail of 16 elements each; checks the tails.  Returns (dz [B,L,L,NZ],
    the 16-bit copy [B,L,L,nz_pad] or None)."""
    B, L, _, NZ = logits.shape
    n32 = B * L * L * NZ
    dz = torch.full((n32 + 16,), SENTINEL, device=DEV)
    n16 = B * L * L * (nz_pad or 0)
    dz16 = torch.full((n16 + 16,), SENTINEL, device=DEV).to(ops.h16()) if nz_pad else None
    p_ = ops.ptr
    rc = _lib.lib.rf_pair_softmax_bwd(p_(logits), p_(datt), datt_ld or L, p_(dz), p_(dz16), nz_pad or 0, B, L, NZ, ops.stream())
    assert rc == 0
    assert (dz[n32:] == SENTINEL).all()
    if nz_pad:
        assert (dz16[n16:].float() == SENTINEL).all()
        dz16 = dz16[:n16].view(B, L, L, nz_pad)
    return dz[:n32].view(B, L, L, NZ), dz16


@pytest.mark.parametrize("shape", SOFTMAX_SHAPES, ids=str)
def test_softmax_bwd_against_float64_autograd(shape, build):
    B, L, NZ = shape
    c = softmax_case(shape)
    ref64, ref32 = softmax_refs(shape)
    dz, _ = run_softmax_bwd(c["logits"], c["datt"])
    assert G.held({"dz": dz.permute(0, 1, 3, 2)}, {"dz": ref64}, {"dz": ref32}, f"{build} pair_softmax_bwd {shape}", **HELD)
    assert torch.equal(ops.pair_softmax_bwd(c["logits"], c["datt"])[0], dz)   # the wrapper: the same bits
    if L == 1:
        assert (dz == 0).all()
    else:   # the check has teeth: the gradient of the transposed maps must fail it
        wrong, _ = run_softmax_bwd(c["logits"], c["datt"].transpose(-1, -2).contiguous())
        assert not G.held({"dz": wrong.permute(0, 1, 3, 2)}, {"dz": ref64}, {"dz": ref32}, "(transposed datt: must fail)", **HELD)
        del RECORDS[-1]


def test_softmax_bwd_ignores_columns_past_the_row(build):
    """datt rows L + 3 apart, the three columns past L poisoned with NaN: the same bits as from the dense gradient"""
    shape = (2, 24, 16)
    B, L, NZ = shape
    c = softmax_case(shape)
    wide = torch.full((NZ, B, L, L + 3), float("nan"), device=DEV)
    wide[..., :L] = c["datt"]
    dense, _ = run_softmax_bwd(c["logits"], c["datt"])
    got, _ = run_softmax_bwd(c["logits"], wide, datt_ld=L + 3)
    assert torch.isfinite(got).all() and torch.equal(got, dense)
    assert torch.isnan(wide[..., L:]).all()   # and nothing was written there
    assert torch.equal(ops.pair_softmax_bwd(c["logits"], wide)[0], dense)


@pytest.mark.parametrize("shape,nz_pad", [((1, 5, 4), 8), ((1, 65, 5), 8), ((2, 24, 16), 16)], ids=str)
def test_softmax_bwd_16_bit_copy(shape, nz_pad, build):
    """the rf_conv_wgrad operand: the fp32 result rounded to the build's 16-bit type, exact zeros in the pad columns, and the
    fp32 output keeps its bits"""
    B, L, NZ = shape
    c = softmax_case(shape)
    alone, _ = run_softmax_bwd(c["logits"], c["datt"])
    dz, dz16 = run_softmax_bwd(c["logits"], c["datt"], nz_pad=nz_pad)
    assert torch.equal(dz, alone)
    assert (dz16[..., NZ:].float() == 0).all()
    assert torch.equal(dz16[..., :NZ], dz.to(ops.h16()))
    w_dz, w_dz16 = ops.pair_softmax_bwd(c["logits"], c["datt"], nz_pad=nz_pad)
    assert torch.equal(w_dz, dz) and torch.equal(w_dz16, dz16)


def test_softmax_bwd_is_deterministic_and_refuses_before_a_launch(build):
    c = softmax_case((1, 257, 16))
    a, _ = run_softmax_bwd(c["logits"], c["datt"])
    b, _ = run_softmax_bwd(c["logits"], c["datt"])
    assert torch.equal(a, b)
    B, L, NZ = 1, 5, 4
    lg, dz = torch.zeros(B, L, L, NZ, device=DEV), torch.zeros(B, L, L, NZ, device=DEV)
    da = torch.zeros(NZ, B, L, L, device=DEV)
    c16 = torch.zeros(B, L, L, 8, device=DEV).to(ops.h16())
    p_ = ops.ptr

    def call(lg_=lg, da_=da, dz_=dz, c16_=None, ld_=L, pad_=0, B_=B, L_=L, NZ_=NZ):
        return _lib.lib.rf_pair_softmax_bwd(p_(lg_), p_(da_), ld_, p_(dz_), p_(c16_), pad_, B_, L_, NZ_, ops.stream())

    assert call() == 0 and call(c16_=c16, pad_=8) == 0
    for name in ("lg_", "da_", "dz_"):
        assert call(**{name: None}) == -1, name       # RF_EINVAL: a NULL tensor
    for name in ("B_", "L_", "NZ_"):
        assert call(**{name: 0}) == -1, name
    assert call(ld_=L - 1) == -1                       # datt_ld < L
    assert call(c16_=c16, pad_=0) == -1                # nz_pad < NZ
    assert call(c16_=c16, pad_=12) == -1               # nz_pad no multiple of 8
    assert call(L_=4096, NZ_=16) == -1                 # a slab beyond the LDS of a compute unit: refused, nothing launched
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.pair_softmax_bwd(lg, da[:, :, :, :4])
    with pytest.raises(ValueError):
        ops.pair_softmax_bwd(lg, da, nz_pad=4)


# ================================================================================================ rf_sym_layernorm_bwd
@functools.lru_cache(maxsize=None)
def sym_case(shape):
    """pair [B,L,L,D] with a per-channel offset and scale (so that the statistics matter), the folded weight [NZ,D], dz"""
    B, L, D, NZ = shape
    g_ = G.gen(6100 + 11 * L + D + NZ)
    pair = torch.randn(B, L, L, D, generator=g_) * (1 + torch.rand(D, generator=g_)) + torch.randn(D, generator=g_)
    w = torch.randn(NZ, D, generator=g_) * D ** -0.5
    dz = torch.randn(B, L, L, NZ, generator=g_)
    return dict(pair=pair.to(DEV), w=w.to(DEV), dz=dz.to(DEV))


def sym_autograd(c, dtype):
    """sum((LayerNorm_no_affine((pair + pair^T) / 2) @ w^T) * dz) differentiated by torch"""
    pair = c["pair"].detach().cpu().to(dtype).clone().requires_grad_()
    s = 0.5 * (pair + pair.transpose(1, 2))
    xhat = torch.nn.functional.layer_norm(s, s.shape[-1:], eps=EPS)
    ((xhat @ c["w"].detach().cpu().to(dtype).t()) * c["dz"].detach().cpu().to(dtype)).sum().backward()
    return pair.grad


@functools.lru_cache(maxsize=None)
def sym_refs(shape):
    c = sym_case(shape)
    return sym_autograd(c, torch.float64), sym_autograd(c, torch.float32)


def run_sym_bwd(c):
    B, L, _, D = c["pair"].shape
    NZ = c["w"].shape[0]
    n = B * L * L * D
    out = torch.full((n + 16,), SENTINEL, device=DEV)
    p_ = ops.ptr
    rc = _lib.lib.rf_sym_layernorm_bwd(p_(c["pair"]), p_(c["dz"]), p_(c["w"]), p_(out), B, L, D, NZ, EPS, ops.stream())
    assert rc == 0
    assert (out[n:] == SENTINEL).all()
    return out[:n].view(B, L, L, D)


@pytest.mark.parametrize("shape", SYM_SHAPES, ids=str)
def test_sym_layernorm_bwd_against_float64_autograd(shape, build):
    c = sym_case(shape)
    ref64, ref32 = sym_refs(shape)
    got = run_sym_bwd(c)
    ref64, ref32 = {"dpair": ref64}, {"dpair": ref32}
    assert G.held({"dpair": got}, ref64, ref32, f"{build} sym_layernorm_bwd {shape}", **HELD)
    assert torch.equal(got, got.transpose(1, 2))                       # dpair[b,i,j] == dpair[b,j,i] bit for bit
    assert torch.equal(run_sym_bwd(c), got)                            # and the same bits on a second run
    assert torch.equal(ops.sym_layernorm_bwd(c["pair"], c["dz"], c["w"], eps=EPS), got)
    # the check has teeth: without the second row of dz (g = dz_ij . w alone) it must fail
    if shape[1] > 1:
        lower = torch.tril(torch.ones(shape[1], shape[1], device=DEV))[None, :, :, None]
        assert not G.held({"dpair": run_sym_bwd(dict(c, dz=c["dz"] * lower))}, ref64, ref32, "(half of dz: must fail)", **HELD)
        del RECORDS[-1]


def test_sym_layernorm_bwd_leaves_its_inputs_alone_and_refuses_before_a_launch(build):
    shape = (2, 5, 72, 12)
    B, L, D, NZ = shape
    c = sym_case(shape)
    keep = {n: c[n].clone() for n in ("pair", "dz", "w")}
    run_sym_bwd(c)
    assert all(torch.equal(c[n], t) for n, t in keep.items())
    out = torch.zeros(B, L, L, D, device=DEV)
    p_ = ops.ptr

    def call(pair_=c["pair"], dz_=c["dz"], w_=c["w"], out_=out, B_=B, L_=L, D_=D, NZ_=NZ, off=0):
        return _lib.lib.rf_sym_layernorm_bwd(p_(pair_, off), p_(dz_), p_(w_), p_(out_), B_, L_, D_, NZ_, EPS, ops.stream())

    assert call() == 0
    for name in ("pair_", "dz_", "w_", "out_"):
        assert call(**{name: None}) == -1, name       # RF_EINVAL: a NULL tensor
    for name in ("B_", "L_", "D_", "NZ_"):
        assert call(**{name: 0}) == -1, name
    assert call(NZ_=65) == -1                          # more than 64 maps
    assert call(D_=30) == -1                           # D no multiple of 4
    assert call(D_=1028) == -1                         # D beyond 1024
    assert call(off=1, B_=1) == -2                     # RF_EALIGN: pair not 16-byte aligned
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.sym_layernorm_bwd(c["pair"], c["dz"][..., :4], c["w"])
    with pytest.raises(ValueError):
        ops.sym_layernorm_bwd(c["pair"][:, :, :4], c["dz"], c["w"])
