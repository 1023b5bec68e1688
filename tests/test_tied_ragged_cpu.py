"""CPU side of the tied attention at any chain length: the entry points with a leading dimension exist in both builds, refuse
what include/rfmi.h says they refuse before anything is launched, and ops.tied_fused_applies refuses what they refuse."""
import ctypes as C

import pytest
import torch

import rosettafold_pytorch_amd as R
from rosettafold_pytorch_amd import _lib, model, ops
from rosettafold_pytorch_amd._lib import I64x3, I64x4

RF_EINVAL, RF_EALIGN = -1, -2
NEW = ("rf_tied_softmax_ld", "rf_tied_logits_ld", "rf_tied_av_ld", "rf_tied_attention_ld")
PTR = C.c_void_p(1 << 20)  # a 16-byte aligned address that is never dereferenced: every call below is refused before a launch


@pytest.fixture(params=[_lib.RF_BF16, _lib.RF_F16], ids=["bf16-build", "f16-build"])
def lib(request):
    return _lib.LIBS[request.param]


def _calls(lib, N=16):
    hs = C.byref(I64x4(0, 0, 32 * 512, 32))
    z3 = C.byref(I64x3(0, 0, 0))
    dt = lib.rf_h16_dtype()
    return {
        "attention": lambda L_, ld: lib.rf_tied_attention_ld(PTR, PTR, PTR, hs, hs, None, z3, 1.0, PTR, ld, None, 0, PTR, hs, 1, 2, N,
                                                             L_, 32, None, 0, None),
        "logits": lambda L_, ld: lib.rf_tied_logits_ld(PTR, PTR, hs, None, z3, 1.0, PTR, ld, None, 0, 1, 2, N, L_, 32, None, 0, None),
        "av": lambda L_, ld: lib.rf_tied_av_ld(PTR, ld, PTR, hs, PTR, hs, 1, 2, N, L_, 32, None),
        "softmax": lambda L_, ld: lib.rf_tied_softmax_ld(PTR, PTR, dt, ld, None, 0, 1, 2, L_, None),
    }


def test_version_and_symbols(lib):
    assert lib.rf_version() >= 12
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.PROTOTYPES


def test_refusals(lib):
    calls = _calls(lib)
    for name, f in calls.items():
        assert f(0, 8) == RF_EINVAL and f(-3, 8) == RF_EINVAL, name                    # L <= 0
        assert f(100, 96) == RF_EINVAL, name                                           # att_ld < L
        assert f(100, 100) == RF_EALIGN and f(100, 108) == RF_EALIGN and f(137, 139) == RF_EALIGN, name  # att_ld % 8
        if name != "softmax":
            assert f(257, 264) == RF_EINVAL and f(300, 304) == RF_EINVAL, name         # L > 256 on the one-pass path


def test_fused_applies_refuses_what_the_library_refuses(lib):
    """(the accepting side needs a device: tests/test_tied_ragged_gpu.py::test_fused_applies_mirrors_the_library)"""
    dt = {_lib.RF_BF16: torch.bfloat16, _lib.RF_F16: torch.float16}[lib.rf_h16_dtype()]
    w = C.c_void_p(1 << 21)
    hs = C.byref(I64x4(0, 0, 32 * 512, 32))
    ws = C.byref(I64x3(0, 0, 512))
    seen = 0
    for L_ in (-1, 0, 1, 63, 64, 100, 192, 200, 256, 257, 300, 512):
        for N in (3, 4, 16, 156, 160, 252, 256, 380, 384):
            if ops.tied_fused_applies(L_, N, dt):
                continue
            ld = ops.tied_ld(max(L_, 1))
            rc = lib.rf_tied_attention_ld(PTR, PTR, PTR, hs, hs, w, ws, 1.0, PTR, ld, None, 0, PTR, hs, 1, 1, N, L_, 32, None, 0, None)
            assert rc == RF_EINVAL, (L_, N, rc)
            seen += 1
            assert not ops.tied_fused_applies(L_, N, torch.float32)
    assert seen >= 40
    assert ops.tied_fused_applies(100, 32, dt) and ops.tied_fused_applies(1, 380, dt) and ops.tied_fused_applies(256, 156, dt)
    assert ops.tied_fused_applies(256, 384, dt, w=False) and not ops.tied_fused_applies(100, 32, dt, dh=64)


def test_leading_dimension_rule():
    """a multiple of 8 keeps its buffers: map_ld(L) == L there, and everywhere in float32"""
    assert [ops.tied_ld(n) for n in (1, 8, 9, 100, 137, 256, 300, 1028)] == [8, 8, 16, 104, 144, 256, 304, 1032]
    try:
        for dt in (torch.bfloat16, torch.float16):
            R.set_compute_dtype(dt)
            assert all(model.map_ld(n) == n for n in range(8, 1100, 8))
            assert model.map_ld(100) == 104 and model.map_ld(1028) == 1032
        R.set_compute_dtype(torch.float32)
        assert all(model.map_ld(n) == n for n in (1, 76, 100, 137, 300))
    finally:
        R.set_compute_dtype(torch.bfloat16)
