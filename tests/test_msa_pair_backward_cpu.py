"""CPU side of the backward through MsaUpdateWithPair and its layer (no GPU): rf_pair_softmax_bwd and rf_sym_layernorm_bwd are
declared in include/rfmi.h, bound by the ctypes table with one argument type per parameter and exported by both builds, the
library says version 18, both classes are RecordingModules of two inputs, enable_backward is per instance and reversible,
switches every layer and each layer's FeedForward along, leaves a second instance and the rest of a block off and leaves the
state_dict alone; and PairUpdateWithMsa still has no enable_backward (the pin of tests/test_outer_backward_cpu.py)."""
import os
import re

import rosettafold_pytorch_amd as R
from rosettafold_pytorch_amd import _lib
from rosettafold_pytorch_amd.model import RecordingModule
from rosettafold_pytorch_amd.structure import TwoTrackBlock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rf_pair_softmax_bwd", "rf_sym_layernorm_bwd")


def _declaration(name):
    with open(os.path.join(ROOT, "include", "rfmi.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    found = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
    assert found, name
    return found.group(1)


def test_entry_points_declared_bound_and_exported():
    kinds = {"int": _lib.i32, "int64_t": _lib.i64, "float": _lib.f32, "uint64_t": _lib.u64}
    for name in NAMES:
        decl = _declaration(name)
        assert name in _lib.PROTOTYPES
        for handle in _lib.LIBS.values():
            assert callable(getattr(handle, name))
            assert handle.rf_version() >= 18
        want = [_lib.vp if "*" in par else kinds[par.split()[-2]] for par in decl.split(",")]
        assert want == _lib.PROTOTYPES[name], name
        assert decl.split(",")[-1].split()[-1] == "stream"   # the stream last, as everywhere in the header
    assert callable(R.ops.pair_softmax_bwd) and callable(R.ops.sym_layernorm_bwd)


def make(layers=3):
    return R.MsaUpdateWithPair(d_msa=32, d_pair=24, n_heads=4, n_encoder_layers=layers, p_dropout=0.0)


def flags(m):
    return [m._rf_backward] + [f for l in m.encoder_layers for f in (l._rf_backward, l.ff.fn[1]._rf_backward)]


def test_both_classes_record_two_inputs():
    for cls in (R.MsaUpdateWithPair, R.MsaUpdateWithPairLayer):
        assert issubclass(cls, RecordingModule)
        assert cls._rf_n_inputs == 2 and cls._rf_scales_own_grads


def test_enable_backward_is_per_instance_reversible_and_switches_the_layers():
    a, b = make(), make()
    assert len(flags(a)) == 7 and not any(flags(a))
    assert a.enable_backward() is a
    assert all(flags(a))
    assert list(a._backward_children()) == list(a.encoder_layers)
    assert not any(flags(b))
    assert a.enable_backward(False) is a
    assert not any(flags(a))


def test_a_layer_switches_its_feed_forward_alone():
    m = make(2)
    first, second = m.encoder_layers
    assert first.enable_backward() is first
    assert first._backward_children() == (first.ff.fn[1],)
    assert first._rf_backward and first.ff.fn[1]._rf_backward
    assert not m._rf_backward and not second._rf_backward and not second.ff.fn[1]._rf_backward
    first.enable_backward(False)
    assert not any(flags(m))


def test_the_other_modules_of_a_block_stay_off():
    blk = TwoTrackBlock(d_msa=96, d_pair=72, n_encoder_layers=2, p_dropout=0.0)
    mu = blk.msa_update_with_pair
    assert mu.enable_backward() is mu
    on = {id(mu)} | {id(x) for l in mu.encoder_layers for x in (l, l.ff.fn[1])}
    for mod in blk.modules():
        assert bool(getattr(mod, "_rf_backward", False)) == (id(mod) in on), type(mod).__name__
    mu.enable_backward(False)
    assert not any(getattr(mod, "_rf_backward", False) for mod in blk.modules())


def test_opting_in_keeps_the_state_dict():
    m = make(2)
    keys = list(m.state_dict())
    m.enable_backward()
    assert list(m.state_dict()) == keys
    assert {"encoder_layers.0.pair2att.1.weight", "encoder_layers.0.pair2att.2.bias", "encoder_layers.1.msa2value.0.bias",
            "encoder_layers.1.msa2value.1.weight", "encoder_layers.0.ff.fn.0.weight", "encoder_layers.1.ff.fn.1.net.0.weight",
            "encoder_layers.1.ff.fn.1.net.3.bias"} <= set(keys)
    lay = R.MsaUpdateWithPairLayer(32, 24, 4, 0.0)
    keys = list(lay.state_dict())
    lay.enable_backward()
    assert list(lay.state_dict()) == keys


def test_pair_update_with_msa_still_has_no_backward():
    """tests/test_outer_backward_cpu.py pins this; the opt-in here does not reach it"""
    assert not hasattr(R.PairUpdateWithMsa, "enable_backward")
