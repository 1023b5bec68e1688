"""CPU side of the pair axial-attention backward (no GPU): the C ABI table of the three new kernels (tests/test_cabi.py ties
header, table and both builds' exports together), and enable_backward's per-module, recursive, reversible switch with its
refusals."""
import pytest

import rosettafold_pytorch_amd as R
from rosettafold_pytorch_amd import _lib

NEW = ("rf_linattn_normalize_bwd", "rf_relu_feature_bwd", "rf_relu_dropout_bwd")
AXIAL = (R.PairUpdateWithAxialAttention, R.PairUpdateWithAxialAttentionLayer, R.PerformerSelfAttention, R.FeedForward)


def test_axial_backward_entry_points_are_bound():
    for name in NEW:
        assert name in _lib.PROTOTYPES
        for lib in _lib.LIBS.values():
            assert callable(getattr(lib, name))
    assert _lib.lib.rf_version() >= 7


def _flags(mod):
    return [m._rf_backward for m in mod.modules() if isinstance(m, AXIAL)]


def test_enable_backward_is_per_module_recursive_and_reversible():
    a = R.PairUpdateWithAxialAttention(32, 64, 2, 0.1, 2)
    b = R.PairUpdateWithAxialAttention(32, 64, 2, 0.1, 2)
    assert a.enable_backward() is a
    fl = _flags(a)
    assert len(fl) == 1 + 2 * 4 and all(fl)
    assert not any(_flags(b))
    a.enable_backward(False)
    assert not any(_flags(a))
    layer = R.PairUpdateWithAxialAttentionLayer(32, 64, 2, 0.1, {})
    assert layer.enable_backward() is layer
    assert layer.row_attn._rf_backward and layer.col_attn._rf_backward and layer.ff._rf_backward
    ff = R.FeedForward(32, 64)
    assert ff.enable_backward() is ff and ff._rf_backward
    pa = R.PerformerSelfAttention(32, heads=2, generalized_attention=True)
    assert pa.enable_backward() is pa and pa._rf_backward


def test_softmax_kernel_performer_refuses_backward():
    pa = R.PerformerSelfAttention(32, heads=2, generalized_attention=False)
    with pytest.raises(NotImplementedError):
        pa.enable_backward()
    assert not pa._rf_backward
    assert pa.enable_backward(False) is pa


def test_model_exposes_the_final_axial_update():
    m = R.RoseTTAFold(d_msa=96, d_pair=72, d_node=8, d_edge=8, d_state=8, n_two_track_blocks=1, n_three_track_blocks=1,
                      n_encoder_layers=1, max_len=64, n_neighbors=[128])
    ax = m.final_block.pair_update_with_axial_attention
    assert ax.enable_backward() is ax
    assert not m.two_track_blocks[0].pair_update_with_axial_attention._rf_backward
