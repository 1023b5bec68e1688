"""CPU side of the fused outer product at any chain length and MSA depth: the rectangular entry point exists in both builds and
refuses what include/rfmi.h says it refuses before anything is launched, OuterProductMean.fused_ok accepts ragged chains and
shallow MSAs in the 16-bit modes only, and ops.outer_operands keeps its shapes unless it is asked for the fused kernel's depth."""
import ctypes as C

import pytest
import torch

import rosettafold_pytorch_amd as R
from rosettafold_pytorch_amd import _lib, ops

RF_EINVAL, RF_EALIGN = -1, -2
PTR = C.c_void_p(1 << 20)   # a 16-byte aligned address that is never dereferenced: every call below is refused before a launch
ODD = C.c_void_p((1 << 20) + 8)


@pytest.fixture(params=[_lib.RF_BF16, _lib.RF_F16], ids=["bf16-build", "f16-build"])
def lib(request):
    return _lib.LIBS[request.param]


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    R.set_compute_dtype(torch.bfloat16)


def test_version_and_symbol(lib):
    assert lib.rf_version() >= 19
    assert "rf_outer_product_ln_linear_rect" in _lib.PROTOTYPES
    assert callable(lib.rf_outer_product_ln_linear_rect)
    assert len(_lib.PROTOTYPES["rf_outer_product_ln_linear_rect"]) == len(_lib.PROTOTYPES["rf_outer_product_ln_linear"]) + 1


def test_refusals(lib):
    def rect(Li=17, Lj=9, N=128, P=32, Dout=288, B=1, xt=PTR, out=PTR, y=None, y_ld=0, g2=None):
        return lib.rf_outer_product_ln_linear_rect(xt, PTR, PTR, PTR, PTR, out, B, Li, Lj, N, P, Dout, 1e-5, g2, g2, 1e-5, y, y_ld, None)
    for kw in ({"Li": 0}, {"Lj": 0}, {"Li": -4}, {"B": 0}, {"P": 16}, {"Dout": 256}, {"N": 100}, {"N": 256}, {"N": 0},
               {"out": None},                               # neither out nor y
               {"y": PTR, "y_ld": 304},                     # y without its LayerNorm
               {"y": PTR, "y_ld": 280, "g2": PTR},          # y_ld < Dout
               {"y": PTR, "y_ld": 300, "g2": PTR},          # y_ld % 8
               {"y": ODD, "y_ld": 304, "g2": PTR}):         # y not 16-byte aligned
        assert rect(**kw) == RF_EINVAL, kw
    assert rect(xt=ODD) == RF_EALIGN and rect(out=ODD) == RF_EALIGN
    # the square entry point is the Li = Lj = L call: the same refusals, and no refusal of a ragged L any more than of a whole one
    sq = lambda L_, N, xt=PTR: lib.rf_outer_product_ln_linear(xt, PTR, PTR, PTR, PTR, PTR, 1, L_, N, 32, 288, 1e-5, None, None,  # noqa: E731
                                                              1e-5, None, 0, None)
    assert sq(0, 128) == RF_EINVAL and sq(17, 100) == RF_EINVAL
    assert sq(17, 128, ODD) == RF_EALIGN and sq(16, 128, ODD) == RF_EALIGN   # (the alignment check comes after every shape check)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_fused_ok_takes_ragged_shapes(dt):
    R.set_compute_dtype(dt)
    m = R.OuterProductMean(32, 288)
    for N, L_ in ((100, 250), (1, 1), (128, 17), (64, 16), (128, 256)):
        assert m.fused_ok(32, N, L_), (N, L_)
    assert not m.fused_ok(32, 129, 250) and not m.fused_ok(32, 256, 256)
    assert not m.fused_ok(16, 100, 250)
    assert not R.OuterProductMean(32, 72).fused_ok(32, 100, 250)
    assert [m.depth_multiple(32, n, 50) for n in (1, 64, 65, 100, 128, 129)] == [64, 64, 128, 128, 128, 8]
    R.RT.fused_outer = False
    try:
        assert not m.fused_ok(32, 100, 250) and m.depth_multiple(32, 100, 250) == 8
    finally:
        R.RT.fused_outer = True


def test_fused_ok_is_false_in_fp32():
    R.set_compute_dtype(torch.float32)
    m = R.OuterProductMean(32, 288)
    assert not m.fused_ok(32, 100, 250) and not m.fused_ok(32, 128, 256)
    assert m.depth_multiple(32, 100, 250) == 8


def test_outer_depth():
    assert [ops.outer_depth(n) for n in (1, 5, 64, 65, 72, 100, 128)] == [64, 64, 64, 128, 128, 128, 128]
    assert ops.outer_depth(129) is None and ops.outer_depth(256) is None


def test_outer_operands_default_shapes(monkeypatch):
    """shapes only: the copies and the fill are device work, replaced here by host allocations"""
    monkeypatch.setattr(ops, "zeros", lambda *s, device=None, dtype=None: torch.zeros(*s, dtype=dtype))
    monkeypatch.setattr(ops, "copy", lambda src, dst: dst)
    for N in (1, 5, 8, 72, 100, 128, 130):
        x = torch.zeros(2, N, 7, 32)
        xt, yt, Np = ops.outer_operands(x, x, torch.bfloat16)
        assert Np == 8 * -(-N // 8)
        assert xt.shape == yt.shape == (2, 7, 32, Np) and xt.dtype == torch.bfloat16
        if N <= 128:
            xt, yt, Np = ops.outer_operands(x, x, torch.bfloat16, ops.outer_depth(N))
            assert Np == (64 if N <= 64 else 128) and xt.shape == (2, 7, 32, Np)


def test_outer_operands_values(monkeypatch):
    """the layout itself, with the copy's contract dst.copy_(src) in the kernel's place: the depth moves innermost, zero-padded"""
    monkeypatch.setattr(ops, "zeros", lambda *s, device=None, dtype=None: torch.zeros(*s, dtype=dtype))
    monkeypatch.setattr(ops, "copy", lambda s, d: d.copy_(s))
    B, N, L_, P = 2, 5, 7, 3
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(B, N, L_, P, generator=g), torch.randn(B, N, L_, P, generator=g)
    xt, yt, Np = ops.outer_operands(x, y, torch.float32)
    assert Np == 8 and xt.shape == yt.shape == (B, L_, P, Np)
    for src, dst in ((x, xt), (y, yt)):
        want = torch.zeros(B, L_, P, Np)
        want[..., :N] = src.permute(0, 2, 3, 1)
        assert torch.equal(dst, want)
