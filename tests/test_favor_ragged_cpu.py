"""The routing predicate of the fused FAVOR+ kernel (ops.favor_fused_applies: the Python mirror of what rf_favor_attention
accepts, plus the model's floor on the sequence length) and the library version that widened the kernel.  No kernel is launched."""
import torch

from rosettafold_pytorch_amd import _lib, ops

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32


def test_library_version():
    assert _lib.lib.rf_version() >= 11


def test_floor_is_one_of_the_measured_candidates():
    assert ops.FAVOR_FUSED_MIN_LS in (16, 32, 48, 64)


def test_predicate_truth_table():
    f = ops.favor_fused_applies
    floor = ops.FAVOR_FUSED_MIN_LS
    for dt in (BF, HF):
        for softmax in (False, True):
            for n in (64, 128, 256):  # the aligned lengths route as they always did
                assert f(n, softmax, 64, 266, dt)
            for n in (65, 72, 100, 137, 200, 255):  # ragged lengths above the floor
                assert f(n, softmax, 64, 266, dt)
            assert f(floor, softmax, 64, 266, dt)
            for n in (1, 8, floor - 1):  # below the floor: the unfused chain
                assert not f(n, softmax, 64, 266, dt)
        for n in (257, 300, 512, 700, 1024):  # beyond one tile: ReLU features only (chunked), the softmax key maximum needs one tile
            assert f(n, False, 64, 266, dt)
            assert not f(n, True, 64, 266, dt)
    for n in (64, 100, 300):
        assert not f(n, False, 64, 266, F32)   # fp32 mode
        assert not f(n, False, 32, 266, BF)    # dim_head != 64
        assert not f(n, False, 64, 256, BF)    # another feature count


def test_floor_can_be_bypassed():
    old = ops.FAVOR_FUSED_MIN_LS
    try:
        ops.FAVOR_FUSED_MIN_LS = 1
        assert ops.favor_fused_applies(1, True, 64, 266, BF) and ops.favor_fused_applies(17, False, 64, 266, HF)
    finally:
        ops.FAVOR_FUSED_MIN_LS = old
