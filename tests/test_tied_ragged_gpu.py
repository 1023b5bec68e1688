"""The tied MSA-row attention at chain lengths that fill no 64 / 128 / 192 / 256 tile (csrc/tied.hip, the TAIL instantiations
behind rf_tied_logits_ld / rf_tied_av_ld / rf_tied_attention_ld) and the general path with a padded leading dimension
(rf_tied_softmax_ld, model.map_ld): kernels against the einsum formulas on the CPU with NaN rows behind every operand and a
sentinel behind every result, refusals, the modules and the whole forward against the oracle, routing and graph capture."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import rosettafold_pytorch_amd as R  # noqa: E402
from oracle import rf_oracle as O  # noqa: E402
from rosettafold_pytorch_amd import _lib, ops  # noqa: E402
from rosettafold_pytorch_amd._lib import I64x3, I64x4  # noqa: E402

DEV = "cuda"
DH = 32
SENTINEL = 12345.0
GUARD = 8  # poisoned rows behind the L rows of every (b, n, h) slab
LENGTHS = [1, 17, 63, 65, 100, 129, 191, 193, 255]
H16 = [torch.bfloat16, torch.float16]
RF_EINVAL, RF_EALIGN = -1, -2


def rel_err(a, b):
    """max |a-b| / max |b|  (tests/test_kernels_gpu.py)"""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-20)).item()


def rel(a, b):
    return rel_err(a, b)


def rn(*s, seed=0):
    return torch.randn(*s, generator=torch.Generator().manual_seed(seed + len(s) + sum(s)))


def state(mod, prefix="m"):
    return {prefix + "." + k: v.detach().float().cpu() for k, v in mod.state_dict().items()}


def build(ctor, seed=11):
    torch.manual_seed(seed)
    return ctor().to(DEV)


@pytest.fixture(params=H16, ids=["bf16", "fp16"])
def h16(request):
    R.set_compute_dtype(request.param)
    yield request.param
    R.set_compute_dtype(torch.bfloat16)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ 1. kernels
def _poisoned(body, fill):
    """body [B, N, G, L, 32] -> the same values as a view of a buffer with GUARD rows of `fill` behind the L rows of every
    (b, n, g) slab"""
    B, N, G, L_, dh = body.shape
    big = torch.full((B, N, G, L_ + GUARD, dh), fill, dtype=body.dtype, device=DEV)
    big[:, :, :, :L_] = body.to(DEV)
    return big, big[:, :, :, :L_]


def _operands(B, H, N, L_, dt, weights):
    g = torch.Generator().manual_seed(1000 * L_ + 10 * N + H)
    qkv = (torch.randn(B, N, 3 * H, L_, DH, generator=g) * (0.9 / math.sqrt(math.sqrt(N)))).to(dt)
    w = torch.rand(B, H, N, L_, generator=g).softmax(2).contiguous() if weights else None
    return qkv, w


def _reference(qkv, w, qs, H, dt):
    """rf.py:252-255 in float64 on the CPU, on the operands the kernel sees (q * w * qscale rounded to the 16-bit type)"""
    q, k = qkv[:, :, :H].float(), qkv[:, :, H:2 * H].float()
    if w is not None:
        q = (q * (w.permute(0, 2, 1, 3).unsqueeze(-1) * qs)).to(dt).float()
    return torch.einsum("bnhid,bnhjd->bhij", q.double(), k.double()).softmax(-1).float()


def _run_ld(B, H, N, L_, dt, weights, att_ld, nan=True):
    """rf_tied_attention_ld on poisoned operands; returns (att [B,H,L,att_ld] + its guard rows, sym, out view, out buffer, qkv, w)"""
    qkv, w = _operands(B, H, N, L_, dt, weights)
    _, view = _poisoned(qkv, float("nan") if nan else 0.0)
    q, k, v = view[:, :, :H], view[:, :, H:2 * H], view[:, :, 2 * H:]
    wd = None
    if weights:  # rows padded to a multiple of 4 floats (16-byte DMA pieces) + GUARD poisoned columns
        Lw = (L_ + 3) // 4 * 4
        wbig = torch.full((B, H, N, Lw + GUARD), float("nan") if nan else 0.0, device=DEV)
        wbig[..., :L_] = w.to(DEV)
        wd = wbig[..., :Lw]
    att_buf = torch.full((B * H * L_ + GUARD, att_ld), SENTINEL, device=DEV, dtype=dt)
    att = att_buf[:B * H * L_].view(B, H, L_, att_ld)
    sym = torch.full((B, L_, L_, H), SENTINEL, device=DEV, dtype=torch.float32)
    out_buf = torch.full((B, N, H, L_ + GUARD, DH), SENTINEL, device=DEV, dtype=dt)
    out = out_buf[:, :, :, :L_]
    qs = 0.37 if weights else 1.0
    ops.tied_attention(q, k, v, out, att, w=wd, qscale=qs, att_sym=sym)
    torch.cuda.synchronize()
    return att_buf, att, sym, out, out_buf, qkv, w, qs


def _check(B, H, N, L_, dt, weights, att_ld):
    att_buf, att, sym, out, out_buf, qkv, w, qs = _run_ld(B, H, N, L_, dt, weights, att_ld)
    a = att.float().cpu()
    want_guard = torch.full((GUARD, att_ld), SENTINEL, dtype=dt)
    # nothing past the chain was written, everything inside was
    assert torch.equal(bits(att_buf[B * H * L_:]), bits(want_guard))
    assert torch.equal(bits(out_buf[:, :, :, L_:]), bits(torch.full((B, N, H, GUARD, DH), SENTINEL, dtype=dt)))
    assert torch.isfinite(a).all() and torch.isfinite(out.float()).all() and torch.isfinite(sym).all()
    assert (a[..., L_:] == 0).all()  # pad columns: exact zeros
    p = a[..., :L_]
    ref_att = _reference(qkv, w, qs, H, dt)
    e_att = rel_err(p, ref_att)
    e_sum = (p.sum(-1) - 1).abs().max().item()
    ref_out = torch.einsum("bhij,bnhjd->bnhid", p.double(), qkv[:, :, 2 * H:].double()).float()  # A.V of the probabilities written
    e_out = rel_err(out, ref_out)
    s = sym.cpu()
    e_sym = rel_err(s, (0.5 * (p + p.transpose(-1, -2))).permute(0, 2, 3, 1))
    print(f"tied ragged L={L_} ld={att_ld} N={N} {dt} w={weights}: att {e_att:.3e} rowsum {e_sum:.3e} out {e_out:.3e} sym {e_sym:.3e}")
    assert e_att < 1.5e-2
    assert e_sum < 2e-2
    assert e_out < 1e-2
    assert e_sym < 1e-6
    assert torch.equal(s, s.transpose(1, 2))
    # the poison reached no result: NaN or zeros behind the operands, the same bits
    _, att0, sym0, out0, _, _, _, _ = _run_ld(B, H, N, L_, dt, weights, att_ld, nan=False)
    assert torch.equal(bits(att), bits(att0)) and torch.equal(bits(out), bits(out0)) and torch.equal(sym.cpu(), sym0.cpu())


@pytest.mark.parametrize("weights", [True, False], ids=["w", "now"])
@pytest.mark.parametrize("L_", LENGTHS)
def test_ragged_kernels(L_, weights, h16):
    """B=1, H=2, N=16: below one MFMA tile, each tile family's first and last ragged length, L % 8 in {1, 3, 4, 7}."""
    _check(1, 2, 16, L_, h16, weights, ops.tied_ld(L_))


def test_ragged_kernels_runs_change_mid_workgroup(h16):
    """B=2, H=3, N=48 at L=100: 288 (b, h, n) units, the (b, h) runs of the persistent attention . V kernel change inside a
    workgroup."""
    _check(2, 3, 48, 100, h16, True, ops.tied_ld(100))


@pytest.mark.parametrize("L_,att_ld", [(100, 264), (64, 72), (128, 136), (200, 256)])
def test_ragged_kernels_other_leading_dimensions(L_, att_ld, h16):
    """att_ld above the tile (the zero fill runs past the strip), a full tile with a padded pitch, att_ld equal to the tile."""
    _check(1, 2, 16, L_, h16, True, att_ld)


@pytest.mark.parametrize("L_", [17, 100, 193, 255])
def test_ragged_av_indexing_is_exact(L_, h16):
    """exact-integer attention . V (row / column / key-order mix-ups show up exactly): bitwise"""
    B, H, N = 1, 2, 16
    ld = ops.tied_ld(L_)
    g = torch.Generator().manual_seed(3 + L_)
    att_i = torch.zeros(B, H, L_, ld, dtype=h16)
    att_i[..., :L_] = torch.randint(0, 3, (B, H, L_, L_), generator=g).to(h16)
    v_i = torch.randint(-2, 3, (B, N, H, L_, DH), generator=g).to(h16)
    _, v = _poisoned(v_i, float("nan"))
    out_buf = torch.full((B, N, H, L_ + GUARD, DH), SENTINEL, device=DEV, dtype=h16)
    ops.tied_av_ld(att_i.to(DEV), v, out_buf[:, :, :, :L_])
    ref_i = torch.einsum("bhij,bnhjd->bnhid", att_i[..., :L_].float(), v_i.float())
    assert torch.equal(out_buf[:, :, :, :L_].float().cpu(), ref_i.to(h16).float())
    assert (out_buf[:, :, :, L_:] == SENTINEL).all()


def _raw_attention(entry, q, k, v, out, att, att_ld, sym, w, qs, ws):
    B, N, H, L_, dh = q.shape
    wst = I64x3(w.stride(0), w.stride(1), w.stride(2)) if w is not None else I64x3(0, 0, 0)
    hs = lambda t: C.byref(I64x4(*t.stride()[:4]))  # noqa: E731
    head = (ops.ptr(q), ops.ptr(k), ops.ptr(v), hs(q), hs(v), ops.ptr(w), C.byref(wst), float(qs), ops.ptr(att))
    tail = (ops.ptr(sym), H, ops.ptr(out), hs(out), B, H, N, L_, dh, ops.ptr(ws), ws.numel() if ws is not None else 0, ops.stream())
    if entry == "ld":
        return _lib.lib.rf_tied_attention_ld(*head, att_ld, *tail)
    return _lib.lib.rf_tied_attention(*head, *tail)


@pytest.mark.parametrize("L_,split", [(128, False), (256, False), (256, True)], ids=["128", "256", "256-split"])
def test_aligned_lengths_are_the_old_entry_points(L_, split, h16):
    """att_ld == L at a full tile: the new entry points run the aligned instantiations (and at 256 the contraction-split form
    when the workspace is given), bit for bit what the old ones give"""
    B, H, N = 1, 2, 16
    qkv, w = _operands(B, H, N, L_, h16, True)
    qkv, w = qkv.to(DEV), w.to(DEV)
    q, k, v = qkv[:, :, :H], qkv[:, :, H:2 * H], qkv[:, :, 2 * H:]
    res = []
    for entry in ("old", "ld"):
        att = torch.empty(B, H, L_, L_, device=DEV, dtype=h16)
        sym = torch.empty(B, L_, L_, H, device=DEV, dtype=torch.float32)
        out = torch.empty(B, N, H, L_, DH, device=DEV, dtype=h16)
        ws = torch.empty(2 * B * H * L_ * L_, device=DEV, dtype=torch.float32) if split else None
        assert _raw_attention(entry, q, k, v, out, att, L_, sym, w, 0.37, ws) == 0
        torch.cuda.synchronize()
        res.append((bits(att), bits(out), sym.cpu()))
    assert all(torch.equal(x, y) for x, y in zip(*res))


# ------------------------------------------------------------------------------------------------ 2. refusals
def test_refusals_and_version(h16):
    assert _lib.lib.rf_version() >= 12
    B, H, N, L_ = 1, 2, 16, 300
    qkv = torch.zeros(B, N, 3 * H, L_, DH, device=DEV, dtype=h16)
    q, k, v = qkv[:, :, :H], qkv[:, :, H:2 * H], qkv[:, :, 2 * H:]
    att = torch.zeros(B * H * L_ * 512, device=DEV, dtype=h16)
    out = torch.zeros(B, N, H, L_, DH, device=DEV, dtype=h16)
    logits = torch.zeros(B * H * L_ * L_, device=DEV, dtype=torch.float32)
    hs = lambda t: C.byref(I64x4(*t.stride()[:4]))  # noqa: E731
    z3 = C.byref(I64x3(0, 0, 0))

    def attention(L__, ld):
        return _lib.lib.rf_tied_attention_ld(ops.ptr(q), ops.ptr(k), ops.ptr(v), hs(q), hs(v), None, z3, 1.0, ops.ptr(att), ld, None,
                                             0, ops.ptr(out), hs(out), B, H, N, L__, DH, None, 0, ops.stream())

    def logits_ld(L__, ld):
        return _lib.lib.rf_tied_logits_ld(ops.ptr(q), ops.ptr(k), hs(q), None, z3, 1.0, ops.ptr(att), ld, None, 0, B, H, N, L__, DH,
                                          None, 0, ops.stream())

    def av(L__, ld):
        return _lib.lib.rf_tied_av_ld(ops.ptr(att), ld, ops.ptr(v), hs(v), ops.ptr(out), hs(out), B, H, N, L__, DH, ops.stream())

    def softmax(L__, ld):
        return _lib.lib.rf_tied_softmax_ld(ops.ptr(logits), ops.ptr(att), ops.dcode(h16), ld, None, 0, B, H, L__, ops.stream())

    for f in (attention, logits_ld, av, softmax):
        assert f(0, 8) == RF_EINVAL and f(-3, 8) == RF_EINVAL     # L <= 0
        assert f(100, 96) == RF_EINVAL                            # att_ld < L
        assert f(100, 100) == RF_EALIGN and f(100, 108) == RF_EALIGN and f(137, 139) == RF_EALIGN  # att_ld % 8
    for f in (attention, logits_ld, av):
        assert f(257, 264) == RF_EINVAL and f(300, 304) == RF_EINVAL  # L > 256: no one-pass kernel, no split form with a pitch
    assert logits_ld(512, 512) == RF_EINVAL   # the split form needs its workspace, as rf_tied_logits
    for f in (attention, logits_ld, av, softmax):
        assert f(100, 104) == 0 and f(1, 8) == 0
    assert softmax(300, 304) == 0             # the general path's softmax takes any L
    torch.cuda.synchronize()


GRID_L = [1, 63, 64, 100, 192, 200, 256, 257, 300]
GRID_N = [3, 4, 16, 156, 160, 380, 384]


def test_fused_applies_mirrors_the_library(h16):
    """ops.tied_fused_applies against rf_tied_attention_ld's return code, with the in-kernel weights, over lengths on both sides of
    256 and MSA depths on both sides of the LDS limit of each tile; float32 has no fused kernel"""
    B, H = 1, 1
    for L_ in GRID_L:
        for N in GRID_N:
            qkv = torch.zeros(B, N, 3 * H, L_, DH, device=DEV, dtype=h16)
            q, k, v = qkv[:, :, :H], qkv[:, :, H:2 * H], qkv[:, :, 2 * H:]
            ld = ops.tied_ld(L_)
            att = torch.zeros(B, H, L_, ld, device=DEV, dtype=h16)
            out = torch.zeros(B, N, H, L_, DH, device=DEV, dtype=h16)
            Lw = (L_ + 3) // 4 * 4
            w = torch.ones(B, H, N, Lw, device=DEV)
            rc = _raw_attention("ld", q, k, v, out, att, ld, None, w, 1.0, None)
            assert (rc == 0) == ops.tied_fused_applies(L_, N, h16), (L_, N, rc)
            assert not ops.tied_fused_applies(L_, N, torch.float32)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. modules against the oracle
MODES = [(torch.float32, 2e-4), (torch.bfloat16, 4e-2), (torch.float16, 6e-3)]  # tests/test_modules_gpu.py


@pytest.fixture(params=MODES, ids=["fp32", "bf16", "fp16"])
def mode(request):
    R.set_compute_dtype(request.param[0])
    yield request.param
    R.set_compute_dtype(torch.bfloat16)


@pytest.fixture
def routes(monkeypatch):
    """launch counters: the fused core (ops.tied_attention, with the att pitch it was given) and the general path's softmax"""
    calls = {"fused": [], "general": [], "w_in_kernel": []}
    fused, general = ops.tied_attention, ops.tied_softmax

    def counted_fused(q, k, v, out, att, **kw):
        calls["fused"].append((q.shape[3], att.shape[3]))
        calls["w_in_kernel"].append(kw.get("w") is not None)
        return fused(q, k, v, out, att, **kw)

    def counted_general(logits, att, *a, **kw):
        calls["general"].append((logits.shape[2], att.shape[3]))
        return general(logits, att, *a, **kw)
    monkeypatch.setattr(ops, "tied_attention", counted_fused)
    monkeypatch.setattr(ops, "tied_softmax", counted_general)
    return calls


DM, NH = 96, 3
MODULE_CASES = [(32, 100), (32, 137), (32, 255), (32, 300), (16, 1028)]
_ORACLE = {}


def _oracle(key, fn):
    """one CPU reference per case, shared by the three modes (the modules are seeded: same weights) and never modified"""
    if key not in _ORACLE:
        _ORACLE[key] = fn()
    return _ORACLE[key]


def _expect_route(routes, mode, Lr):
    h16_mode = mode[0] != torch.float32
    if h16_mode and Lr <= 256:
        assert routes["fused"] == [(Lr, ops.tied_ld(Lr))] and routes["general"] == [], routes
    else:
        assert routes["fused"] == [] and routes["general"] == [(Lr, ops.tied_ld(Lr) if h16_mode else Lr)], routes


@pytest.mark.parametrize("N,Lr", MODULE_CASES)
def test_soft_tied_attention_ragged(N, Lr, mode, routes):
    m = build(lambda: R.SoftTiedAttentionOverResidues(DM, NH, 0.0, return_att=True))
    x = rn(1, N, Lr, DM)
    ro, ra = _oracle(("tied", N, Lr), lambda: O.soft_tied_attention(state(m), "m", x, NH))
    out, att = m(x.to(DEV))
    _expect_route(routes, mode, Lr)
    e_o, e_a = rel(out, ro), rel(att, ra)
    print(f"soft tied L={Lr} N={N} {mode[0]}: out {e_o:.3e} att {e_a:.3e}")
    assert e_o < mode[1] and e_a < mode[1]
    assert torch.equal(att, att.transpose(1, 2))


@pytest.mark.parametrize("N,Lr", MODULE_CASES)
def test_tied_encoder_layer_ragged(N, Lr, mode, routes):
    m = build(lambda: R.EncoderLayer(d_msa=DM, d_ff=4 * DM, n_heads=NH, p_dropout=0.0, tied=True, return_att=True))
    x = rn(1, N, Lr, DM)
    ro, ra = _oracle(("enc", N, Lr), lambda: O.encoder_layer_tied(state(m), "m", x, NH))
    out, att = m(x.to(DEV))
    _expect_route(routes, mode, Lr)
    e_o, e_a = rel(out, ro), rel(att, ra)
    print(f"tied encoder L={Lr} N={N} {mode[0]}: out {e_o:.3e} att {e_a:.3e}")
    assert e_o < mode[1] and e_a < mode[1]
    assert torch.equal(att, att.transpose(1, 2))


def test_soft_tied_attention_ragged_with_folded_weights(h16, routes):
    """d_msa 384, 12 heads, 128 x 137 rows: the q|k|v projection goes to the register-resident-weights GEMM, which folds the
    position weights into q on its accumulators (rows of w 137 floats apart), and the logits kernel runs without them"""
    N, Lr, D, H = 128, 137, 384, 12
    m = build(lambda: R.SoftTiedAttentionOverResidues(D, H, 0.0, return_att=True))
    x = rn(1, N, Lr, D)
    ro, ra = _oracle(("tied384",), lambda: O.soft_tied_attention(state(m), "m", x, H))
    out, att = m(x.to(DEV))
    assert routes["fused"] == [(Lr, ops.tied_ld(Lr))] and routes["general"] == [], routes
    assert routes["w_in_kernel"] == [not ops.gemm_takes_row_scale(N * Lr, 3 * D, D)] == [False]
    tol = 4e-2 if h16 == torch.bfloat16 else 6e-3  # tests/test_modules_gpu.py
    e_o, e_a = rel(out, ro), rel(att, ra)
    print(f"soft tied folded L={Lr} N={N} {h16}: out {e_o:.3e} att {e_a:.3e}")
    assert e_o < tol and e_a < tol
    assert torch.equal(att, att.transpose(1, 2))


def test_msa_update_with_pair_ragged(mode):
    N, Lr, DP = 8, 100, 72
    m = build(lambda: R.MsaUpdateWithPair(DM, DP, 4, n_encoder_layers=2, p_dropout=0.0))
    msa, pair = rn(1, N, Lr, DM), rn(1, Lr, Lr, DP)
    ref = _oracle(("msa_pair",), lambda: O.msa_update_with_pair(state(m), "m", msa, pair, 2, 4))
    e = rel(m(msa.to(DEV), pair.to(DEV)), ref)
    print(f"msa update with pair L={Lr} {mode[0]}: {e:.3e}")
    assert e < mode[1]


def test_tied_row_attention_op_takes_a_ragged_length():
    """the dispatcher op keeps its schema and runs the ragged case through the new entry points"""
    import rosettafold_pytorch_amd.custom_ops  # noqa: F401  (registers torch.ops.rfmi.*)
    R.set_compute_dtype(torch.bfloat16)
    B, N, Lr, H = 1, 16, 100, 4
    q, k, v = ((rn(B, N, Lr, H, DH, seed=s_) * 0.4).bfloat16() for s_ in (0, 1, 2))
    att = torch.einsum("bnihd,bnjhd->bhij", q.float(), k.float()).softmax(-1)
    ref = torch.einsum("bhij,bnjhd->bnihd", att, v.float()).reshape(B, N, Lr, H * DH)
    out, sym = torch.ops.rfmi.tied_row_attention(q.to(DEV), k.to(DEV), v.to(DEV))
    # (bounds of tests/test_kernels_gpu.py::test_tied_row_attention_functional_and_custom_op)
    assert rel_err(out, ref) < 2e-2 and rel_err(sym, (0.5 * (att + att.transpose(-1, -2))).permute(0, 2, 3, 1)) < 1.5e-2


# ------------------------------------------------------------------------------------------------ 4. whole model
# tests/test_favor_ragged_gpu.py's CFG on the smooth path (tests/test_modules_gpu.py::test_full_model_smooth_path_bf16_tolerance)
CFG = dict(d_input=21, d_msa=96, d_pair=72, d_node=8, d_edge=8, d_state=8, n_two_track_blocks=1, n_three_track_blocks=1,
           n_encoder_layers=2, max_len=80, n_neighbors=[128], p_dropout=0.1)
FULL_N, FULL_L = 32, 76


def _full_inputs():
    g = torch.Generator().manual_seed(61)
    msa = torch.randint(0, 21, (1, FULL_N, FULL_L), generator=g)
    return msa, msa[:, 0].clone(), torch.arange(FULL_L).unsqueeze(0)


def _full_model():
    torch.manual_seed(5)
    return R.RoseTTAFold(**CFG).to(DEV).eval()


def test_full_model_ragged_length(mode, routes):
    """L = 76 (L % 8 == 4, above the FAVOR+ floor): rel-L2 of the four logit maps below 6e-2 in the 16-bit modes, 5e-4 in fp32"""
    model = _full_model()
    msa, seq, aa = _full_inputs()

    def ref():
        P = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
        return O.rosettafold_forward(P, msa, seq, aa, CFG)[0]
    rl = _oracle(("full",), ref)
    with torch.no_grad():
        logits, xyz, plddt = model(msa.to(DEV), seq.to(DEV), aa.to(DEV))
    # (d_msa 96 over the model's 12 heads: d_head 8, no fused kernel -- every tied attention of the forward takes the general
    # path, in the 16-bit modes with the padded pitch)
    ld = FULL_L if mode[0] == torch.float32 else ops.tied_ld(FULL_L)
    assert routes["general"] and all(c == (FULL_L, ld) for c in routes["general"]) and not routes["fused"], routes
    tol = 5e-4 if mode[0] == torch.float32 else 6e-2
    errs = {}
    for k_ in ("theta", "phi", "dist", "omega"):
        a, b = logits[k_].double().cpu(), rl[k_].double()
        errs[k_] = ((a - b).norm() / b.norm()).item()
    print(f"full model L={FULL_L} {mode[0]}: rel-L2 {errs}")
    for t in list(logits.values()) + [xyz, plddt]:
        assert torch.isfinite(t).all()
    assert all(e < tol for e in errs.values()), errs


def test_ragged_forward_captures_into_a_graph():
    """nothing on the ragged route reads back from the device: the bf16 forward captures, and replays bitwise the eager forward"""
    R.set_compute_dtype(torch.bfloat16)
    model = _full_model()
    a = tuple(t.to(DEV) for t in _full_inputs())

    def flat(out):
        return [out[0][k] for k in sorted(out[0])] + [out[1], out[2]]
    eager = [t.clone() for t in flat(model(*a))]
    gf = R.GraphedForward(model, *a)
    for _ in range(2):
        assert all(torch.equal(x, y) for x, y in zip(flat(gf(*a)), eager))
