"""CPU-side checks of the OuterProductMean backward pass: the new entry points are declared, bound and exported by both builds,
and enable_backward() is a per-module, reversible switch that an enclosing PairUpdateWithMsa does not see.  No kernel is
launched."""
import rosettafold_pytorch_amd as R
from rosettafold_pytorch_amd import _lib

NEW = ("rf_layernorm_bwd_fused", "rf_layernorm_bwd_fused_ws_bytes")


def test_new_entry_points_bound_in_both_builds():
    for name in NEW:
        assert name in _lib.PROTOTYPES
        for handle in _lib.LIBS.values():
            assert callable(getattr(handle, name))
    assert _lib.lib.rf_version() >= 9


def test_workspace_query_needs_no_device():
    for handle in _lib.LIBS.values():
        assert handle.rf_layernorm_bwd_fused_ws_bytes(70, 1024) >= 2 * 1024 * 4
        assert handle.rf_layernorm_bwd_fused_ws_bytes(0, 1024) == 0


def test_enable_backward_is_per_module_and_reversible():
    a, b = R.OuterProductMean(4, 16), R.OuterProductMean(4, 16)
    assert not a._rf_backward and not b._rf_backward
    assert a.enable_backward() is a
    assert a._rf_backward and not b._rf_backward
    assert a.enable_backward(False) is a
    assert not a._rf_backward


def test_enclosing_module_is_untouched():
    pum = R.PairUpdateWithMsa(d_msa=16, d_proj=4, d_pair=16, n_heads=2)
    pum.outer_product_mean.enable_backward()
    assert pum.outer_product_mean._rf_backward
    assert not getattr(pum, "_rf_backward", False)
    assert not hasattr(pum, "enable_backward")
    other = R.PairUpdateWithMsa(d_msa=16, d_proj=4, d_pair=16, n_heads=2)
    assert not other.outer_product_mean._rf_backward


def test_one_input_modules_keep_one_input():
    assert R.FeedForward(8, 16)._rf_n_inputs == 1 and R.OuterProductMean(4, 16)._rf_n_inputs == 2
