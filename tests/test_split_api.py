"""CPU checks of the "high" float32 matmul precision (split-bf16 GEMMs, RF_F32X3): the setting, the header constant, and which
rf_gemm operand code a float32 GEMM carries in every mode.  No kernel is launched: rf_gemm is replaced by a recorder."""
import ast
import ctypes
import os
import re

import pytest
import torch

import rosettafold_pytorch_amd as R
from rosettafold_pytorch_amd import _lib as L
from rosettafold_pytorch_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def restore_modes():
    yield
    R.set_float32_matmul_precision("highest")
    R.set_compute_dtype(torch.bfloat16)


def test_default_is_highest():
    assert R.get_float32_matmul_precision() == "highest"


def test_set_get_and_reject(restore_modes):
    R.set_float32_matmul_precision("high")
    assert R.get_float32_matmul_precision() == "high"
    R.set_float32_matmul_precision("highest")
    assert R.get_float32_matmul_precision() == "highest"
    for bad in ("medium", "HIGH", "", None, 3):
        with pytest.raises(ValueError):
            R.set_float32_matmul_precision(bad)
    assert R.get_float32_matmul_precision() == "highest"


def test_header_defines_the_code():
    src = open(os.path.join(ROOT, "include", "rfmi.h")).read()
    m = re.search(r"#define\s+RF_F32X3\s+(\d+)", src)
    assert m and int(m.group(1)) == L.RF_F32X3 == 3
    assert len({L.RF_F32, L.RF_BF16, L.RF_F16, L.RF_F32X3}) == 4


class _Recorder:
    def __init__(self):
        self.codes = []

    def rf_gemm(self, d, stream):
        self.codes.append(ctypes.cast(d, ctypes.POINTER(L.GemmDesc)).contents.ab_dtype)
        return 0


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(ops, "lib", rec)
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)
    monkeypatch.setattr(ops, "stream", lambda: None)
    return rec


def _f32_gemm(exact=False):
    A, B, C = torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4, 4)
    ops.gemm(A, B, C, 4, 4, 8, exact=exact)
    ops.linear(A, B, out=C, exact=exact)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("precision", ["highest", "high"])
def test_float32_gemm_code(recorder, restore_modes, dtype, precision):
    # both orders of the two setters give the same routing
    R.set_float32_matmul_precision(precision)
    R.set_compute_dtype(dtype)
    _f32_gemm()
    R.set_compute_dtype(dtype)
    R.set_float32_matmul_precision(precision)
    _f32_gemm()
    split = dtype == torch.float32 and precision == "high"
    assert recorder.codes == [L.RF_F32X3 if split else L.RF_F32] * 4
    recorder.codes.clear()
    _f32_gemm(exact=True)  # a pinned call stays exact in every mode
    assert recorder.codes == [L.RF_F32] * 2
    if dtype != torch.float32:  # 16-bit operands keep their own code
        recorder.codes.clear()
        h = torch.zeros(4, 8, dtype=dtype)
        ops.gemm(h, h, torch.zeros(4, 4), 4, 4, 8)
        assert recorder.codes == [ops.dcode(dtype)]


def test_gemm_code_table(restore_modes):
    R.set_compute_dtype(torch.float32)
    R.set_float32_matmul_precision("high")
    assert ops.gemm_code(torch.float32) == L.RF_F32X3
    assert ops.gemm_code(torch.float32, exact=True) == L.RF_F32
    assert ops.gemm_code(torch.bfloat16) == L.RF_BF16
    R.set_compute_dtype(torch.bfloat16)
    assert ops.gemm_code(torch.float32) == L.RF_F32
    R.set_compute_dtype(torch.float32)
    assert ops.gemm_code(torch.float32) == L.RF_F32X3  # the stored setting comes back with the float32 mode
    R.set_float32_matmul_precision("highest")
    assert ops.gemm_code(torch.float32) == L.RF_F32


def _calls(path, names):
    tree = ast.parse(open(path).read())
    out = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in names:
            if isinstance(node.func.value, ast.Name) and node.func.value.id == "ops":
                out.append(node)
    return out


def test_structure_track_states_its_precision():
    """Every contraction of structure.py says whether it follows the float32 precision (exact=False: the T()-typed
    operands of the MSA update) or stays exact (exact=True: the fp32-by-design structure track); the SE(3) stack, the
    coordinate update and the pLDDT head are all pinned."""
    path = os.path.join(ROOT, "rosettafold-pytorch_amd", "structure.py")
    calls = _calls(path, {"gemm", "linear"})
    assert len(calls) >= 10
    kw = {}
    for c in calls:
        v = [k.value for k in c.keywords if k.arg == "exact"]
        assert len(v) == 1 and isinstance(v[0], ast.Constant), f"structure.py:{c.lineno} does not state exact="
        kw[c.lineno] = v[0].value
    assert sum(kw.values()) >= 10
    follow = [ln for ln, e in kw.items() if not e]
    assert len(follow) == 2, follow  # MsaUpdateWithPairAndCoord: value projection and attention . V in the compute dtype
