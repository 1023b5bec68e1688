"""CPU side of the backward through MsaEmbedding and PairEmbedding (no GPU): rf_embedding_bwd and rf_pair_axis_sums are declared
in include/rfmi.h, bound by the ctypes table with one argument type per parameter and exported by both builds, the library says
version 21, the workspace queries answer 0 for an empty problem and grow with the shape, both classes are RecordingModules of
two and three inputs, enable_backward is per instance, reversible and leaves the state_dict alone, a RoseTTAFold's
msa_emb.enable_backward() switches nothing else on, and PairUpdateWithMsa still has no enable_backward (the pin of
tests/test_outer_backward_cpu.py)."""
import os
import re

import rosettafold_pytorch_amd as R
from rosettafold_pytorch_amd import _lib
from rosettafold_pytorch_amd.model import RecordingModule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rf_embedding_bwd", "rf_pair_axis_sums")


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
        assert name in _lib.PROTOTYPES and name + "_ws_bytes" in _lib.PROTOTYPES
        for handle in _lib.LIBS.values():
            assert callable(getattr(handle, name)) and callable(getattr(handle, name + "_ws_bytes"))
            assert handle.rf_version() >= 21
        want = [_lib.vp if "*" in par else kinds[par.split()[-2]] for par in decl.split(",")]
        assert want == _lib.PROTOTYPES[name], name
        assert decl.split(",")[-1].split()[-1] == "stream"   # the stream last, as everywhere in the header
    assert callable(R.ops.embedding_bwd) and callable(R.ops.pair_axis_sums)


def test_workspace_queries():
    for handle in _lib.LIBS.values():
        emb, pas = handle.rf_embedding_bwd_ws_bytes, handle.rf_pair_axis_sums_ws_bytes
        for empty in ((0, 32, 21), (8, 0, 21), (8, 32, 0), (-1, 32, 21)):
            assert emb(*empty) == 0, empty
        for empty in ((0, 8, 32), (1, 0, 32), (1, 8, 0)):
            assert pas(*empty) == 0, empty
        assert emb(8, 32, 127) == 0   # a table whose sums do not fit the LDS the kernel enables: refused, like the call
        one = emb(1, 8, 21)
        assert one == 23 * 8 * 8       # one fp64 partial [V + 2, D]
        assert emb(1024, 8, 21) == one < emb(1025, 8, 21) < emb(1 << 20, 8, 21)
        assert emb(1, 16, 21) == 2 * one and emb(1, 8, 44) == 2 * one
        small = pas(1, 2, 8)
        assert 0 < small < pas(2, 2, 8) < pas(2, 13, 8) < pas(2, 13, 40) < pas(2, 257, 40)
        assert isinstance(emb(4 * 128 * 256, 384, 21), int) and pas(4, 256, 288) > 2 ** 25   # an int64 answer


def test_both_classes_record_their_inputs():
    for cls, n in ((R.MsaEmbedding, 2), (R.PairEmbedding, 3)):
        assert issubclass(cls, RecordingModule)
        assert cls._rf_n_inputs == n


def make():
    return (R.MsaEmbedding(d_input=21, d_msa=32, max_len=64), R.PairEmbedding(d_input=21, d_pair=32, max_len=64),
            R.PairEmbedding(d_input=21, d_pair=32, max_len=64, use_template=True, d_template=16))


def test_enable_backward_is_per_instance_and_reversible():
    for a, b in zip(make(), make()):
        assert not a._rf_backward and not b._rf_backward
        assert a.enable_backward() is a
        assert a._rf_backward and not b._rf_backward
        assert tuple(a._backward_children()) == ()
        assert not any(getattr(m, "_rf_backward", False) for m in a.modules() if m is not a)
        assert a.enable_backward(False) is a
        assert not a._rf_backward


def test_opting_in_keeps_the_state_dict():
    msa, pair, templ = make()
    for mod, want in ((msa, {"to_embedding.weight", "query_enc.weight"}),
                      (pair, {"embed_seq.weight", "proj.weight", "proj.bias"}),
                      (templ, {"embed_seq.weight", "proj.weight", "proj.bias", "ln_template.weight", "ln_template.bias"})):
        keys = list(mod.state_dict())
        mod.enable_backward()
        assert list(mod.state_dict()) == keys and set(keys) == want
        assert [n for n, _ in mod.named_parameters()] == keys   # the order _RecordedFn spreads the gradients in


def test_the_models_embedding_switches_nothing_else():
    model = R.RoseTTAFold(d_input=21, d_msa=96, d_pair=72, d_node=8, d_edge=8, d_state=8, n_two_track_blocks=1,
                          n_three_track_blocks=1, n_encoder_layers=1, max_len=64, n_neighbors=[128], p_dropout=0.0)
    keys = list(model.state_dict())
    assert model.msa_emb.enable_backward() is model.msa_emb
    on = [m for m in model.modules() if getattr(m, "_rf_backward", False)]
    assert on == [model.msa_emb]
    assert list(model.state_dict()) == keys
    model.msa_emb.enable_backward(False)
    assert not any(getattr(m, "_rf_backward", False) for m in model.modules())


def test_pair_update_with_msa_still_has_no_backward():
    """tests/test_outer_backward_cpu.py pins this; the opt-in here does not reach it"""
    assert not hasattr(R.PairUpdateWithMsa, "enable_backward")
