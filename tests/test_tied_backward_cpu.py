"""CPU side of the backward through SoftTiedAttentionOverResidues (no GPU): rf_tied_softmax_bwd and rf_scale_rows_bwd are
declared in include/rfmi.h, bound by the ctypes table with one argument type per parameter and exported by both builds, the
library says version 17, and enable_backward on the module is per instance, reversible, switches `poswise_weight` along,
leaves an EncoderLayer around an un-switched module off and leaves the state_dict alone."""
import os
import re

import pytest

import rosettafold_pytorch_amd as R
from rosettafold_pytorch_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rf_tied_softmax_bwd", "rf_scale_rows_bwd")


def _declaration(name):
    with open(os.path.join(ROOT, "include", "rfmi.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    found = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
    assert found, name
    return found.group(1)


@pytest.mark.parametrize("name", NAMES)
def test_entry_point_declared_bound_and_exported(name):
    decl = _declaration(name)
    assert name in _lib.PROTOTYPES
    for handle in _lib.LIBS.values():
        assert callable(getattr(handle, name))
        assert handle.rf_version() >= 17
    kinds = {"int": _lib.i32, "int64_t": _lib.i64, "float": _lib.f32, "uint64_t": _lib.u64}
    want = [_lib.vp if "*" in par else kinds[par.split()[-2]] for par in decl.split(",")]
    assert want == _lib.PROTOTYPES[name]
    assert decl.split(",")[-1].split()[-1] == "stream"   # the stream last, as everywhere in the header
    assert callable(getattr(R.ops, name[3:]))


def make():
    return R.SoftTiedAttentionOverResidues(d_msa=32, n_heads=2, p_dropout=0.0)


def flags(m):
    return [m._rf_backward, m.poswise_weight._rf_backward]


def test_enable_backward_is_per_instance_reversible_and_switches_the_position_weights():
    a, b = make(), make()
    assert isinstance(a, R.model.RecordingModule) and type(a)._rf_n_inputs == 1
    assert not any(flags(a))
    assert a.enable_backward() is a
    assert all(flags(a))
    assert a._backward_children() == (a.poswise_weight,)
    assert not any(flags(b))
    assert a.enable_backward(False) is a
    assert not any(flags(a))


def test_an_encoder_layer_around_an_unswitched_module_stays_off():
    layer = R.EncoderLayer(d_msa=32, d_ff=64, n_heads=2, p_dropout=0.0, tied=True)
    other = make().enable_backward()
    assert all(flags(other))
    assert not any(getattr(mod, "_rf_backward", False) for mod in layer.modules())
    attn = layer.attn
    assert attn.enable_backward() is attn
    on = {id(attn), id(attn.poswise_weight)}
    for mod in layer.modules():
        assert bool(getattr(mod, "_rf_backward", False)) == (id(mod) in on), type(mod).__name__
    attn.enable_backward(False)
    assert not any(getattr(mod, "_rf_backward", False) for mod in layer.modules())


def test_opting_in_keeps_the_state_dict():
    m = make()
    keys = list(m.state_dict())
    m.enable_backward()
    assert list(m.state_dict()) == keys
    assert {"poswise_weight.to_q.0.weight", "poswise_weight.to_k.0.bias", "to_q.weight", "to_k.bias", "to_v.weight",
            "to_out.bias"} <= set(keys)
