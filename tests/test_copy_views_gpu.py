"""ops.copy on the device: the battery of tests/test_copy_views_cpu.py through rf_copy4d in both libraries and every dtype pair,
exact against dst.copy_(src) on the host; the destination's storage outside the view keeps its sentinel."""
import pytest
import torch

import rosettafold_pytorch_amd as R
from rosettafold_pytorch_amd import ops
from test_copy_views_cpu import SENTINEL, _storage, battery

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def h16(request):
    R.set_compute_dtype(request.param)
    yield request.param
    R.set_compute_dtype(torch.bfloat16)


def _as(view, dtype, device):
    """the same view over a copy of its whole storage, in another dtype and on another device"""
    return torch.as_strided(_storage(view).clone().to(dtype).to(device), view.shape, view.stride(), view.storage_offset())


@pytest.mark.parametrize("name", sorted(battery()))
def test_copy_matches_host(h16, name):
    src, dst = battery()[name]
    src = _as(src, F32, "cpu")
    _storage(src).div_(3).add_(0.125)          # finite values that neither 16-bit type holds exactly
    for x_dt, y_dt in ((F32, F32), (F32, h16), (h16, F32), (h16, h16)):
        src_h, dst_h = _as(src, x_dt, "cpu"), _as(dst, y_dt, "cpu")
        src_d, dst_d = _as(src_h, x_dt, "cuda"), _as(dst_h, y_dt, "cuda")
        dst_h.copy_(src_h)
        out = ops.copy(src_d, dst_d)
        torch.cuda.synchronize()
        assert out is dst_d
        got, want = _storage(dst_d).cpu(), _storage(dst_h)
        assert torch.equal(got, want), (name, x_dt, y_dt)
        assert int((want != SENTINEL).sum()) == dst.numel()   # (so the comparison above covers the sentinel everywhere else)
