"""CPU side of the backward through PositionWiseWeightFactor and InitialCoordGenerationWithMsaAndPair (no GPU): rf_poswise_bwd
is declared in include/rfmi.h, bound by the ctypes table with one argument type per parameter and exported by both builds, the
library says version 15, and enable_backward on the coordinate module is per instance, reversible, switches every block and
its `attn` along and leaves the state_dict alone."""
import os
import re

import rosettafold_pytorch_amd as R
from rosettafold_pytorch_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rf_poswise_bwd",)


def test_entry_point_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "rfmi.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.PROTOTYPES
        for handle in _lib.LIBS.values():
            assert callable(getattr(handle, name))
        # one argument type per parameter of the declaration
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.PROTOTYPES[name]), name
    for handle in _lib.LIBS.values():
        assert handle.rf_version() >= 15


def test_prototype_follows_the_declaration_type_by_type():
    with open(os.path.join(ROOT, "include", "rfmi.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    decl = re.search(r"\bint\s+rf_poswise_bwd\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
    kinds = {"int": _lib.i32, "int64_t": _lib.i64, "float": _lib.f32, "uint64_t": _lib.u64}
    want = [_lib.vp if "*" in par else kinds[par.split()[-2]] for par in decl.split(",")]
    assert want == _lib.PROTOTYPES["rf_poswise_bwd"]


def make():
    return R.InitialCoordGenerationWithMsaAndPair(16, 16, d_node=8, d_edge=8, n_heads=4, n_layers=2, p_dropout=0.0)


def flags(m):
    return [m._rf_backward] + [b._rf_backward for b in m.blocks] + [b.attn._rf_backward for b in m.blocks]


def test_enable_backward_is_per_instance_reversible_and_switches_the_blocks():
    a, b = make(), make()
    assert not any(flags(a))
    assert a.enable_backward() is a
    assert all(flags(a)) and len(flags(a)) == 5
    assert not any(flags(b))
    assert a.enable_backward(False) is a
    assert not any(flags(a))
    # the shared softmax front opts in on its own: the coordinate module differentiates it through _node_input_backward
    p = R.PositionWiseWeightFactor(24, 3, 0.0)
    q = R.PositionWiseWeightFactor(24, 3, 0.0)
    assert not p._rf_backward
    assert p.enable_backward() is p and p._rf_backward and not q._rf_backward
    assert not p.enable_backward(False)._rf_backward


def test_opting_in_keeps_the_state_dict():
    m = make()
    keys = list(m.state_dict())
    m.enable_backward()
    assert list(m.state_dict()) == keys
    assert {"ln_msa.weight", "poswise_weight.to_k.0.bias", "node_embed.0.weight", "edge_embed.0.bias",
            "blocks.1.attn.edge_emb.weight", "to_out.bias"} <= set(keys)
    p = R.PositionWiseWeightFactor(24, 3, 0.0)
    keys = list(p.state_dict())
    assert list(p.enable_backward().state_dict()) == keys == ["to_q.0.weight", "to_q.0.bias", "to_k.0.weight", "to_k.0.bias"]
