"""ops.copy on the host: ops.copy_walk turns two views of one shape into the (dims, xs, ys) that rf_copy4d walks.  A reference
interpreter of copy4d_kernel's index arithmetic (csrc/ops.hip), applied to the two storages at the views' storage offsets, must
reproduce dst.copy_(src) exactly for every layout pattern the model uses; what ops.copy refuses, it refuses before any launch."""
import pytest
import torch

from rosettafold_pytorch_amd import _lib, ops

SENTINEL = -7.0


def _storage(t):
    """the whole storage of a view's base tensor, as a flat tensor sharing memory with it"""
    return torch.as_strided(t, (t.untyped_storage().nbytes() // t.element_size(),), (1,), 0)


def kernel_copy(src, dst):
    """copy4d_kernel on the host: the flat index e runs row-major over the padded dims of ops.copy_walk"""
    dims, xs, ys = ops.copy_walk(src.shape, src.stride(), dst.stride())
    assert len(dims) <= 4
    pad = 4 - len(dims)
    dims, xs, ys = (1,) * pad + dims, (0,) * pad + xs, (0,) * pad + ys
    x, y = _storage(src), _storage(dst)
    for e in range(dims[0] * dims[1] * dims[2] * dims[3]):
        i3, t = e % dims[3], e // dims[3]
        i2, t = t % dims[2], t // dims[2]
        i1, i0 = t % dims[1], t // dims[1]
        y[dst.storage_offset() + i0 * ys[0] + i1 * ys[1] + i2 * ys[2] + i3 * ys[3]] = \
            x[src.storage_offset() + i0 * xs[0] + i1 * xs[1] + i2 * xs[2] + i3 * xs[3]]


def _rand(*shape):
    return torch.arange(1, 1 + torch.Size(shape).numel(), dtype=torch.float32).view(*shape)


def _blank(*shape):
    return torch.full(shape, SENTINEL)


def battery():
    """name -> (src view, dst view); every dimension of a case differs, so that a swapped stride cannot hide"""
    cases = {}
    x = _rand(2, 5, 7, 3)
    cases["middle_transpose"] = (x.transpose(1, 2), _blank(2, 7, 5, 3))
    cases["middle_transpose_dst"] = (x, _blank(2, 7, 5, 3).transpose(1, 2))
    cases["column_slice"] = (x, _blank(2, 5, 7, 11)[..., 4:7])
    m = _rand(2, 9, 6)
    cases["broadcast_rows"] = (m[:, 2:6, None, :].expand(2, 4, 9, 6), _blank(2, 4, 9, 16)[..., 3:9])
    cases["broadcast_columns"] = (m[:, None, :, :].expand(2, 4, 9, 6), _blank(2, 4, 9, 16)[..., 9:15])
    cases["outer_operands"] = (_rand(2, 5, 7, 3).permute(0, 2, 3, 1), _blank(2, 7, 3, 8)[..., :5])      # N = 5 into Np = 8
    hs, Lr, P, Kx = 2, 5, 3, 16                                                                          # Kx = pad8(Lr * P)
    cases["slice_unflatten"] = (_rand(hs, Lr, P, P), _blank(hs * P, Kx).view(hs, P, Kx)[..., :Lr * P].unflatten(2, (Lr, P))
                                .permute(0, 2, 1, 3))
    cases["y_n"] = (_rand(Lr, P, 8), _blank(8, Kx)[:, :Lr * P].unflatten(1, (Lr, P)).permute(1, 2, 0))
    cases["five_dims_merging"] = (_rand(2, 3, 4, 5, 6).transpose(2, 3), _blank(2, 3, 5, 4, 6))
    cases["five_dims_sample"] = (_rand(2, 3, 4, 5, 6)[1].permute(0, 3, 1, 2), _blank(2, 3, 6, 4, 5)[1])
    cases["row_of_a_matrix"] = (_rand(6, 4)[2:5].t(), _blank(4, 3))
    return cases


@pytest.mark.parametrize("name", sorted(battery()))
def test_walk_reproduces_copy(name):
    src, dst = battery()[name]
    want_base = _storage(dst).clone()
    want = torch.as_strided(want_base, dst.shape, dst.stride(), dst.storage_offset())
    want.copy_(src)
    kernel_copy(src, dst)
    assert torch.equal(_storage(dst), want_base)           # the view holds src, every other element still the sentinel
    assert torch.equal(dst, src.expand_as(dst))
    assert int((_storage(dst) != SENTINEL).sum()) == dst.numel()


def test_walk_drops_and_merges():
    assert ops.copy_walk((1, 1, 6, 4), (0, 0, 4, 1), (0, 0, 4, 1)) == ((24,), (1,), (1,))
    assert ops.copy_walk((2, 3, 4), (12, 4, 1), (24, 8, 1)) == ((6, 4), (4, 1), (8, 1))        # the left pair merges on both sides
    assert ops.copy_walk((2, 3, 4), (12, 4, 1), (12, 1, 3)) == ((2, 3, 4), (12, 4, 1), (12, 1, 3))
    assert ops.copy_walk((2, 1, 3), (3, 99, 1), (3, 7, 1)) == ((6,), (1,), (1,))               # a size-1 stride never matters
    assert ops.copy_walk((2, 4, 3), (0, 0, 1), (12, 3, 1)) == ((8, 3), (0, 1), (3, 1))         # a broadcast merges with itself
    assert ops.copy_walk((), (), ()) == ((), (), ())


def test_walk_runs_on_meta_tensors():
    a, b = torch.empty(2, 5, 7, 3, device="meta"), torch.empty(2, 7, 5, 3, device="meta")
    assert ops.copy_walk(a.transpose(1, 2).shape, a.transpose(1, 2).stride(), b.stride()) == ((2, 7, 5, 3), (105, 3, 21, 1),
                                                                                             (105, 15, 3, 1))


class _Refused(Exception):
    pass


@pytest.fixture
def no_launch(monkeypatch):
    """host tensors stand in for device tensors: the checks under test come before the library call, which must not happen"""
    def launch(*a):
        raise _Refused("rf_copy4d reached")
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)
    monkeypatch.setattr(ops, "stream", lambda: None)
    monkeypatch.setattr(ops, "lib", type("Lib", (), {"rf_copy4d": staticmethod(launch)})())


def test_refusals(no_launch):
    with pytest.raises(ValueError, match="shapes differ"):
        ops.copy(torch.zeros(2, 3), torch.zeros(3, 2))
    with pytest.raises(ValueError, match="needs 5 dimensions"):
        ops.copy(torch.zeros(2, 3, 4, 5, 6).permute(4, 3, 2, 1, 0), torch.zeros(6, 5, 4, 3, 2))
    with pytest.raises(ValueError, match="repeats elements"):
        ops.copy(torch.zeros(2, 3), torch.zeros(3).expand(2, 3))
    with pytest.raises(TypeError):
        ops.copy(torch.zeros(2, 3, dtype=torch.float64), torch.zeros(2, 3))
    with pytest.raises(_lib.RfmiError):   # the 16-bit type of the other library
        ops.copy(torch.zeros(2, 3, dtype=torch.float16), torch.zeros(2, 3))
    with pytest.raises(_Refused):         # what passes every check reaches the library
        ops.copy(torch.zeros(2, 3, 4, 5, 6).transpose(2, 3), torch.zeros(2, 3, 5, 4, 6))
    with pytest.raises(_Refused):         # a size-1 destination dimension may have any stride
        ops.copy(torch.zeros(1, 3), torch.zeros(3).expand(1, 3))


def test_copy_needs_device_tensors():
    with pytest.raises(_lib.RfmiError):
        ops.copy(torch.zeros(2, 3), torch.zeros(2, 3))
