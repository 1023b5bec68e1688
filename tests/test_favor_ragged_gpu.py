"""The fused FAVOR+ kernel at sequence lengths that are no multiple of its 64 / 128 / 256-row tiles (csrc/favor.hip, the TAIL
instantiations): against the CPU oracle and the unfused kernel chain, with NaN guard rows around q|k|v and a sentinel around the
output (rows past the end of a sequence are neither read nor written), through the model's routing predicate, under hipGraph
capture and on the 4-wave kernel."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import rosettafold_pytorch_amd as R  # noqa: E402
from oracle import rf_oracle as O  # noqa: E402
from rosettafold_pytorch_amd import _lib, ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
DP, H = 72, 3
INNER, W3 = 64 * H, 3 * 64 * H
SM_LENGTHS = [1, 17, 63, 65, 100, 127, 129, 200, 255]
RELU_LENGTHS = SM_LENGTHS + [257, 300, 511, 513, 700]


def rel(a, b):
    """max |a-b| / max |b|"""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-20)).item()


def rel2(a, b):
    """relative L2 error ||a-b|| / ||b||"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def rn(*s, seed=0):
    return torch.randn(*s, generator=torch.Generator().manual_seed(seed + len(s) + sum(s)))


def state(mod, prefix="m"):
    return {prefix + "." + k: v.detach().float().cpu() for k, v in mod.state_dict().items()}


def build(ctor, seed=11):
    torch.manual_seed(seed)
    return ctor().to(DEV)


@pytest.fixture
def no_floor(monkeypatch):
    """the model's floor on the sequence length is a routing decision, not a limit of the kernel: bypass it"""
    monkeypatch.setattr(ops, "FAVOR_FUSED_MIN_LS", 1)


@pytest.fixture
def counter(monkeypatch):
    calls = []
    inner = ops.favor_attention

    def counted(*a, **k):
        calls.append(a[11])  # seq_len
        return inner(*a, **k)
    monkeypatch.setattr(ops, "favor_attention", counted)
    return calls


_ORACLE = {}


def _oracle(m, generalized, n):
    """one CPU reference per (feature map, length), shared by both 16-bit modes (the module is seeded: same weights) and never
    modified"""
    if (generalized, n) not in _ORACLE:
        _ORACLE[generalized, n] = O.performer_self_attention(state(m), "m", rn(5, n, DP), H, generalized)
    return _ORACLE[generalized, n]


# ------------------------------------------------------------------------------------------------ 1. module vs oracle / unfused chain
@pytest.mark.parametrize("generalized,n", [(False, n) for n in SM_LENGTHS] + [(True, n) for n in RELU_LENGTHS])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_ragged_fused_favor_attention(generalized, n, dt, no_floor, counter):
    """The pattern and the bounds of test_modules_gpu.test_fused_favor_attention at ragged lengths: a single row, a partial
    16-row tile, a partial s-block pair, an all-padding tile, all-padding phase-B waves, every tile size from just below and
    just above, a partial last chunk of 2 and 3 chunks.
    The unfused chain keeps its sequences contiguous in k'^T and v^T, so in the 16-bit modes it answers RF_EALIGN to every
    length that is no multiple of 8 (of these lengths it runs 200 only): there it has no error to assert, and the fused route
    is held to the same bounds against the oracle alone."""
    R.set_compute_dtype(dt)
    try:
        m = build(lambda: R.PerformerSelfAttention(dim=DP, heads=H, generalized_attention=generalized))
        x = rn(5, n, DP)
        ref = _oracle(m, generalized, n)
        R.RT.fused_favor = True
        y_f = m(x.to(DEV))
        assert counter == [n]  # the fused kernel ran, once
        R.RT.fused_favor = False
        try:
            y_u = m(x.to(DEV))
        except _lib.RfmiError as e:  # rejected arguments: nothing was launched
            assert "RF_EALIGN" in str(e) and n % 8 != 0, e
            y_u = None
        assert counter == [n]
        R.RT.fused_favor = True
        tol = 4e-2 if generalized else 4.5e-2
        l2 = 2e-2
        if dt == torch.float16:
            tol, l2 = 6e-3, 3e-3
        ef, ef2 = rel(y_f, ref), rel2(y_f, ref)
        eu = rel(y_u, ref) if y_u is not None else None
        print(f"favor ragged gen={generalized} n={n} {dt}: unfused {eu} fused {ef:.3e} fused-L2 {ef2:.3e}")
        assert torch.isfinite(y_f).all()
        if y_u is not None:
            assert eu < tol
        assert ef < tol, (ef, eu)
        assert ef2 < l2
    finally:
        R.RT.fused_favor = True
        R.set_compute_dtype(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ raw launches
def _proj(gen):
    m = build(lambda: R.PerformerSelfAttention(dim=DP, heads=H, generalized_attention=gen))
    return m.proj_scaled(log2e=not gen)


def _layout(strided, n, Lo):
    """(x_strides, o_strides, row of (sequence o, position s), rows a 256-row tile of over-reach could touch)"""
    if strided:  # sequences along axis 1 of [n, Lo] rows: sequence stride Lo rows, outer stride one row
        return (n * Lo * W3, W3, Lo * W3, 64), (n * Lo * INNER, INNER, Lo * INNER), (lambda o, s: s * Lo + o), 256 * Lo
    return (Lo * n * W3, n * W3, W3, 64), (Lo * n * INNER, n * INNER, INNER), (lambda o, s: o * n + s), 256


def _launch(qkv, pc, out, xs, os_, Lo, n, gen):
    ops.favor_attention(qkv, pc, out, xs, os_, 0, INNER, 2 * INNER, 1, Lo, H, n, 64, 266, not gen, 1e-3 if gen else 1e-4)


RAW_CASES = [(False, 65), (False, 100), (True, 65), (True, 100), (True, 300)]


# ------------------------------------------------------------------------------------------------ 2. guards
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("gen,n", RAW_CASES)
def test_nothing_outside_the_sequence_is_read_or_written(gen, n, strided):
    """q|k|v sits in the middle of a buffer whose guard rows are NaN, the output in a buffer filled with a sentinel.  The guards
    are as large as a whole 256-row tile of over-reach, so a wrong kernel is observed, not provoked into a fault."""
    Lo = 3
    R.set_compute_dtype(torch.bfloat16)
    xs, os_, _, guard = _layout(strided, n, Lo)
    rows = n * Lo
    pc = _proj(gen)
    body = torch.randn(rows, W3, generator=torch.Generator().manual_seed(n)).bfloat16().to(DEV)
    sentinel = 12345.0

    def run(guard_value):
        big = torch.full((guard + rows + guard, W3), guard_value, device=DEV, dtype=torch.bfloat16)
        big[guard:guard + rows] = body
        obig = torch.full((guard + rows + guard, INNER), sentinel, device=DEV, dtype=torch.bfloat16)
        _launch(big[guard:guard + rows], pc, obig[guard:guard + rows], xs, os_, Lo, n, gen)
        torch.cuda.synchronize()
        return obig
    o_nan = run(float("nan"))
    o_zero = run(0.0)
    want = torch.full((guard, INNER), sentinel, dtype=torch.bfloat16).view(torch.int16)
    assert torch.equal(o_nan[:guard].cpu().view(torch.int16), want)
    assert torch.equal(o_nan[guard + rows:].cpu().view(torch.int16), want)
    inside = o_nan[guard:guard + rows]
    assert torch.isfinite(inside.float()).all()
    assert not (inside == sentinel).all(dim=1).any()  # every row of every sequence was written
    assert torch.equal(inside.view(torch.int16), o_zero[guard:guard + rows].view(torch.int16))


# ------------------------------------------------------------------------------------------------ 3. neighbours
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("gen,n", RAW_CASES)
def test_sequences_do_not_see_their_neighbours(gen, n, strided):
    """Only sequence 1 of 3 changes: the outputs of sequences 0 and 2 stay bitwise what they were (a key mask or a row clamp
    that is off by a tile would let rows of the neighbour in)."""
    Lo = 3
    R.set_compute_dtype(torch.bfloat16)
    xs, os_, row, _ = _layout(strided, n, Lo)
    pc = _proj(gen)
    g = torch.Generator().manual_seed(7 + n)
    qkv = torch.randn(n * Lo, W3, generator=g).bfloat16()
    qkv2 = qkv.clone()
    mine = torch.tensor([row(1, s) for s in range(n)])
    qkv2[mine] = (3.0 * torch.randn(n, W3, generator=g)).bfloat16()
    outs = []
    for t in (qkv, qkv2):
        o = torch.zeros(n * Lo, INNER, device=DEV, dtype=torch.bfloat16)
        _launch(t.to(DEV), pc, o, xs, os_, Lo, n, gen)
        outs.append(o.cpu().view(torch.int16))
    others = torch.tensor([row(o, s) for o in (0, 2) for s in range(n)])
    assert torch.equal(outs[0][others], outs[1][others])
    assert not torch.equal(outs[0][mine], outs[1][mine])


# ------------------------------------------------------------------------------------------------ 4. run to run
@pytest.mark.parametrize("gen,n", [(False, 100), (False, 200), (True, 100), (True, 200), (True, 300)])
def test_ragged_run_to_run(gen, n):
    Lo = 40  # 120 items
    R.set_compute_dtype(torch.bfloat16)
    xs, os_, _, _ = _layout(False, n, Lo)
    pc = _proj(gen)
    qkv = torch.randn(Lo * n, W3, generator=torch.Generator().manual_seed(3)).bfloat16().to(DEV)
    outs = []
    for _ in range(3):
        o = torch.empty(Lo * n, INNER, device=DEV, dtype=torch.bfloat16)
        _launch(qkv, pc, o, xs, os_, Lo, n, gen)
        outs.append(o)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


# ------------------------------------------------------------------------------------------------ 5. routing and layers
def test_axial_layer_routes_ragged_rows_and_columns(counter):
    """72 x 72 pair picture: both axial attentions (strided rows, contiguous columns) run the fused kernel; bound of
    test_modules_gpu.test_fused_favor_axis1_strides."""
    R.set_compute_dtype(torch.bfloat16)
    m = build(lambda: R.PairUpdateWithAxialAttentionLayer(DP, 4 * DP, 8, 0.0, {}))
    x = rn(1, 72, 72, DP)
    ref = O.pair_axial_layer(state(m), "m", x, 8)
    y = m(x.to(DEV))
    assert counter == [72, 72]
    assert rel(y, ref) < 4e-2


def test_performer_encoder_layer_routes_ragged_msa_columns(counter):
    """72 MSA rows attended per residue column (seq_axis = 1: strided sequences) against the oracle's Performer encoder layer,
    which attends along dim 2 of its input: the transposed problem."""
    R.set_compute_dtype(torch.bfloat16)
    m = build(lambda: R.EncoderLayer(d_msa=96, d_ff=4 * 96, n_heads=12, p_dropout=0.0, tied=False, performer=True))
    x = rn(1, 72, 16, 96)
    ref = O.encoder_layer_performer(state(m), "m", x.transpose(1, 2).contiguous(), 12).transpose(1, 2)
    y = x.to(DEV).clone()  # the fp32 residual stream, updated in place
    m.run(y, seq_axis=1)
    assert counter == [72]
    assert rel(y, ref) < 4e-2  # test_modules_gpu's bound of the bf16 mode


def test_below_the_floor_and_fp32_stay_unfused(counter):
    assert ops.FAVOR_FUSED_MIN_LS in (16, 32, 48, 64)
    m = build(lambda: R.PerformerSelfAttention(dim=DP, heads=H, generalized_attention=True))
    R.set_compute_dtype(torch.bfloat16)
    m(rn(2, ops.FAVOR_FUSED_MIN_LS - 8, DP).to(DEV))  # (a multiple of 8: the 16-bit unfused chain takes no other length)
    assert counter == []
    m(rn(2, ops.FAVOR_FUSED_MIN_LS, DP).to(DEV))
    assert counter == [ops.FAVOR_FUSED_MIN_LS]
    R.set_compute_dtype(torch.float32)
    try:
        m(rn(2, 104, DP).to(DEV))
    finally:
        R.set_compute_dtype(torch.bfloat16)
    assert counter == [ops.FAVOR_FUSED_MIN_LS]


# ------------------------------------------------------------------------------------------------ 6. 4-wave kernel
_CHILD = r"""
import sys, torch
sys.path.insert(0, {root!r})
import rosettafold_pytorch_amd as R
from oracle import rf_oracle as O
R.set_compute_dtype(torch.bfloat16)
for n in (100, 200, 300):
    torch.manual_seed(11)
    m = R.PerformerSelfAttention(dim=72, heads=3, generalized_attention=True).to("cuda")
    x = torch.randn(5, n, 72, generator=torch.Generator().manual_seed(n))
    ref = O.performer_self_attention({{"m." + k: v.detach().float().cpu() for k, v in m.state_dict().items()}}, "m", x, 3, True)
    R.RT.fused_favor = True
    y_f = m(x.to("cuda")).float().cpu()
    err = ((y_f - ref).abs().max() / ref.abs().max()).item()
    l2 = ((y_f - ref).double().norm() / ref.double().norm()).item()
    print("RF_FAVOR4 n", n, "fused vs oracle", err, l2, flush=True)
    assert torch.isfinite(y_f).all() and err < 4e-2 and l2 < 2e-2, (err, l2)
    if n % 8 == 0:  # the 16-bit unfused chain takes multiples of 8 only
        R.RT.fused_favor = False
        y_u = m(x.to("cuda")).float().cpu()
        eu = ((y_u - ref).abs().max() / ref.abs().max()).item()
        d = ((y_f - y_u).abs().max() / y_u.abs().max()).item()
        print("RF_FAVOR4 n", n, "unfused vs oracle", eu, "fused vs unfused", d, flush=True)
        assert eu < 4e-2 and d < 4e-2 + eu, (eu, d)
"""


def test_four_wave_kernel_in_a_fresh_process():
    """RF_FAVOR4 is read once per process: a child with the switch set runs the ReLU features at 100, 200 and 300 rows.  The
    16-bit unfused chain refuses 100 and 300 (RF_EALIGN: no multiples of 8), so the reference at every length is the oracle
    under the bf16 bounds of test_ragged_fused_favor_attention; at 200 the unfused chain is compared too (by the triangle
    inequality the two routes are no further apart than the sum of their distances to the oracle)."""
    env = dict(os.environ, RF_FAVOR4="1")
    r = subprocess.run(["timeout", "-k", "10", "150", sys.executable, "-c", _CHILD.format(root=ROOT)], env=env, cwd=ROOT,
                       capture_output=True, text=True)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert all(f"RF_FAVOR4 n {n} fused vs oracle" in r.stdout for n in (100, 200, 300))


# ------------------------------------------------------------------------------------------------ 7. graph capture
# tests/test_axial_backward_gpu.py's CFG, with max_len raised to hold 72 residues
CFG = dict(d_input=21, d_msa=96, d_pair=72, d_node=8, d_edge=8, d_state=8, n_two_track_blocks=1, n_three_track_blocks=1,
           n_encoder_layers=2, max_len=80, n_neighbors=[128], p_dropout=0.1)


def test_ragged_forward_captures_into_a_graph(counter):
    """L = 72 and 72 MSA rows: both tracks route to the fused kernel; nothing in the route reads back from the device, so the
    forward still captures, and the replay is bitwise the eager forward."""
    R.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(5)
    model = R.RoseTTAFold(**CFG).to(DEV).eval()
    g = torch.Generator().manual_seed(61)
    msa = torch.randint(0, 21, (1, 72, 72), generator=g)
    a = (msa.to(DEV), msa[:, 0].clone().to(DEV), torch.arange(72).unsqueeze(0).to(DEV))

    def flat(out):
        return [out[0][k] for k in sorted(out[0])] + [out[1], out[2]]
    eager = [t.clone() for t in flat(model(*a))]
    assert counter and all(n == 72 for n in counter)
    gf = R.GraphedForward(model, *a)
    for _ in range(2):
        assert all(torch.equal(x, y) for x, y in zip(flat(gf(*a)), eager))


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refused_lengths():
    R.set_compute_dtype(torch.bfloat16)
    qkv = torch.zeros(512, W3, device=DEV, dtype=torch.bfloat16)
    out = torch.zeros(512, INNER, device=DEV, dtype=torch.bfloat16)
    pc = _proj(False)

    def rc(n, softmax):
        xs = _lib.I64x4(512 * W3, 0, W3, 64)
        os_ = _lib.I64x3(512 * INNER, 0, INNER)
        return _lib.lib.rf_favor_attention(ops.ptr(qkv), ops.ptr(pc), ops.ptr(out), C.byref(xs), C.byref(os_), 0, INNER, 2 * INNER,
                                           1, 1, H, n, 64, 266, softmax, 1e-3, ops.stream())
    assert rc(0, 0) == -1 and rc(0, 1) == -1 and rc(-5, 0) == -1  # RF_EINVAL
    assert rc(257, 1) == -1
    assert rc(257, 0) == 0 and rc(256, 1) == 0 and rc(1, 1) == 0
    torch.cuda.synchronize()
