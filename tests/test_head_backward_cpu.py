"""CPU side of the PredictionHead / ResNet backward (no GPU): the repacked kernel of a convolution's input gradient, and the
C ABI table of the three new kernels (tests/test_cabi.py ties header, table and both builds' exports together)."""
import pytest
import torch
import torch.nn.functional as F

from rosettafold_pytorch_amd import _lib
from rosettafold_pytorch_amd.model import conv_input_grad_weight


@pytest.mark.parametrize("dilation", [1, 2, 4, 8])
def test_conv_input_grad_is_a_conv_with_the_repacked_kernel(dilation):
    g = torch.Generator().manual_seed(dilation)
    Co, Ci, H, W = 5, 3, 19, 23
    w = torch.randn(Co, Ci, 3, 3, generator=g, dtype=torch.float64)
    dy = torch.randn(2, Co, H, W, generator=g, dtype=torch.float64)
    ref = torch.nn.grad.conv2d_input((2, Ci, H, W), w, dy, padding=dilation, dilation=dilation)
    got = F.conv2d(dy, conv_input_grad_weight(w), padding="same", dilation=dilation)
    assert got.shape == ref.shape
    assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12)


def test_one_by_one_repack_is_the_transpose():
    w = torch.randn(7, 4, 1, 1, dtype=torch.float64)
    assert torch.equal(conv_input_grad_weight(w)[:, :, 0, 0], w[:, :, 0, 0].t())


def test_backward_entry_points_are_bound():
    for name in ("rf_conv_wgrad", "rf_instnorm_bwd", "rf_layernorm_bwd"):
        assert name in _lib.PROTOTYPES
    assert _lib.lib.rf_version() >= 6


def test_enable_backward_is_per_module_and_recursive():
    import rosettafold_pytorch_amd as R
    a, b = R.PredictionHead(64, 2, 0.1), R.PredictionHead(64, 2, 0.1)
    assert a.enable_backward() is a
    blocks = [m for m in a.modules() if isinstance(m, (R.ResNet, R.ResBlock2D))]
    assert len(blocks) == 4 * 3 and all(m._rf_backward for m in blocks)
    assert not any(m._rf_backward for m in b.modules() if isinstance(m, (R.PredictionHead, R.ResNet, R.ResBlock2D)))
    a.enable_backward(False)
    assert not any(m._rf_backward for m in a.modules() if isinstance(m, (R.PredictionHead, R.ResNet, R.ResBlock2D)))
    r = R.ResNet(1, 16, 16, 8)
    assert r.enable_backward() is r and r.layer[3]._rf_backward
