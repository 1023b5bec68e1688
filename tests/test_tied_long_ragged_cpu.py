"""CPU side of the tied attention at any chain length to 1024 and any MSA depth (no GPU): both builds say version 20 and export
rf_tied_logits_long and rf_tied_logits_long_ws_elems, the ctypes table binds them with one type per parameter of the header's
declarations, and ops.tied_long_applies mirrors the split rule of the entry point."""
import ctypes as C
import os
import re

import torch

from rosettafold_pytorch_amd import _lib, ops
from rosettafold_pytorch_amd.runtime import RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rf_tied_logits_long", "rf_tied_logits_long_ws_elems")


def _declaration(name):
    with open(os.path.join(ROOT, "include", "rfmi.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    found = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
    assert found, name
    return found.group(1), found.group(2)


def test_both_builds_say_version_20_and_export_the_entry_points():
    for handle in _lib.LIBS.values():
        assert handle.rf_version() >= 20
        for name in NAMES:
            assert callable(getattr(handle, name))
    for path in (_lib.LIB_PATH, _lib.LIB16_PATH):  # exported by the files themselves, not only bound by the table
        raw = C.CDLL(path)
        assert all(hasattr(raw, name) for name in NAMES), path


def test_prototypes_match_the_header_parameter_for_parameter():
    kinds = {"int": _lib.i32, "int64_t": _lib.i64, "float": _lib.f32}

    def ctype(par):
        if "[4]" in par:
            return C.POINTER(_lib.I64x4)
        return _lib.vp if "*" in par else kinds[par.split()[-2]]
    for name in NAMES:
        ret, decl = _declaration(name)
        assert [ctype(par) for par in decl.split(",")] == _lib.PROTOTYPES[name], name
        for handle in _lib.LIBS.values():
            assert getattr(handle, name).restype == (C.c_int64 if ret == "int64_t" else C.c_int), name
    assert _declaration("rf_tied_logits_long")[1].split(",")[-1].split()[-1] == "stream"
    # no position weights on long rows: the entry point is rf_tied_logits_ld without w / w_strides
    ld = list(_lib.PROTOTYPES["rf_tied_logits_ld"])
    assert _lib.PROTOTYPES["rf_tied_logits_long"] == ld[:3] + ld[5:]


def test_tied_long_applies_mirrors_the_split_rule():
    for dt in (torch.bfloat16, torch.float16):
        for L, N in [(257, 4), (300, 64), (1023, 128), (1000, 136)]:
            assert ops.tied_long_applies(L, N, dt), (L, N)
        # L outside 257 .. 1024; N odd; 132 = 4 ranges of 33 rows (an odd range)
        for L, N in [(256, 64), (1025, 64), (300, 7), (300, 132)]:
            assert not ops.tied_long_applies(L, N, dt), (L, N)
        assert not ops.tied_long_applies(300, 64, dt, dh=64)
    assert not ops.tied_long_applies(300, 64, torch.float32)
    assert callable(ops.tied_logits_long) and "tied_logits_long" in ops.COUNTERS
    assert isinstance(RT.tied_long_ragged, bool)
