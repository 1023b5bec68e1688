"""CPU side of the backward through MsaUpdateWithPairAndCoord (no GPU): rf_dist_masked_attention_bwd is declared in
include/rfmi.h, bound by the ctypes table with one argument type per parameter and exported by both builds, the library says
version 16, and enable_backward on the module is per instance, reversible, switches the FeedForward of `to_out` along, leaves
the other modules of a ThreeTrackBlock off and leaves the state_dict alone."""
import os
import re

import rosettafold_pytorch_amd as R
from rosettafold_pytorch_amd import _lib
from rosettafold_pytorch_amd.structure import ThreeTrackBlock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rf_dist_masked_attention_bwd"


def _declaration():
    with open(os.path.join(ROOT, "include", "rfmi.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    found = re.search(r"\bint\s+" + NAME + r"\s*\((.*?)\)\s*;", header, flags=re.S)
    assert found, NAME
    return found.group(1)


def test_entry_point_declared_bound_and_exported():
    decl = _declaration()
    assert NAME in _lib.PROTOTYPES
    for handle in _lib.LIBS.values():
        assert callable(getattr(handle, NAME))
        assert handle.rf_version() >= 16
    kinds = {"int": _lib.i32, "int64_t": _lib.i64, "float": _lib.f32, "uint64_t": _lib.u64}
    want = [_lib.vp if "*" in par else kinds[par.split()[-2]] for par in decl.split(",")]
    assert want == _lib.PROTOTYPES[NAME]
    assert decl.split(",")[-1].split()[-1] == "stream"   # the stream last, as everywhere in the header
    assert callable(R.ops.dist_masked_attention_bwd)


def make():
    return R.MsaUpdateWithPairAndCoord(d_msa=32, d_state=16, d_trfm_inner=32, d_ff=64, p_dropout=0.0)


def flags(m):
    return [m._rf_backward, m.to_out.fn[1]._rf_backward]


def test_enable_backward_is_per_instance_reversible_and_switches_the_feed_forward():
    a, b = make(), make()
    assert type(a)._rf_n_inputs == 3
    assert not any(flags(a))
    assert a.enable_backward() is a
    assert all(flags(a))
    assert a._backward_children() == (a.to_out.fn[1],)
    assert not any(flags(b))
    assert a.enable_backward(False) is a
    assert not any(flags(a))


def test_the_other_modules_of_a_three_track_block_stay_off():
    blk = ThreeTrackBlock(d_msa=96, d_pair=72, d_node=8, d_edge=8, d_state=8, n_encoder_layers=1, n_neighbors=8, p_dropout=0.0)
    mu = blk.msa_update_with_pair_and_coord
    assert mu.enable_backward() is mu
    on = {id(mu), id(mu.to_out.fn[1])}
    for mod in blk.modules():
        assert bool(getattr(mod, "_rf_backward", False)) == (id(mod) in on), type(mod).__name__
    mu.enable_backward(False)
    assert not any(getattr(mod, "_rf_backward", False) for mod in blk.modules())


def test_opting_in_keeps_the_state_dict():
    m = make()
    keys = list(m.state_dict())
    m.enable_backward()
    assert list(m.state_dict()) == keys
    assert {"ln_msa.weight", "ln_state.bias", "to_q.weight", "to_k.bias", "to_v.weight", "ln_out.weight", "to_out.fn.0.weight",
            "to_out.fn.1.net.0.weight", "to_out.fn.1.net.3.bias"} <= set(keys)
