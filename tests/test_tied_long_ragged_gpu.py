"""The fused tied MSA-row attention at any chain length to 1024 and any MSA depth to 256 (csrc/tied.hip):

  rf_tied_logits_long    the tail instantiations of the contraction-split logits kernel and of its softmax, per element against the
                         float64 oracle of tests/attn_oracle.py with the FACTOR and the allowances of
                         tests/test_attn_bound_gpu.py::run_logits, in both 16-bit builds, on NaN-padded operands (tied_case: NaN
                         rows behind every (b, n, h) slab) and a sentinel-filled result; whole tiles bit for bit rf_tied_logits;
                         refusals
  rf_poswise_collapsed   the tail instantiations (N off a multiple of 16) against the same oracle as run_poswise
  the module             SoftTiedAttentionOverResidues against oracle/rf_oracle.py on the new routes, the switch, one recorded
                         backward against float64 autograd, graph capture."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import attn_oracle as A  # noqa: E402
import grad_oracle as G  # noqa: E402
import rosettafold_pytorch_amd as R  # noqa: E402
from oracle import rf_oracle as O  # noqa: E402
from rosettafold_pytorch_amd import _lib, ops  # noqa: E402
from rosettafold_pytorch_amd.runtime import RT  # noqa: E402
from grad_oracle import h16  # noqa: E402,F401  (the fixture: both 16-bit builds)

lib = _lib.lib
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
P = ops.ptr
EINVAL, EALIGN = -1, -2
SENTINEL = 12345.0


def dn(dt):
    return {torch.bfloat16: "bf16", torch.float16: "fp16"}[dt]


def i4(v):
    return C.byref(_lib.I64x4(*[int(x) for x in v]))


def nkb(L):
    return (L + 255) // 256


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


@pytest.fixture(autouse=True)
def _restore():
    yield
    R.set_compute_dtype(torch.bfloat16)
    RT.tied_long_ragged = True


# ================================================================================================ rf_tied_logits_long
def run_long(B, H, N, L, h, *, att_ld=None, spread=4.0, seed=0, entry="long"):
    """tests/test_attn_bound_gpu.py::run_logits for the long entry point: the same oracle, FACTOR and allowances.  q / k sit in
    NaN storage with three NaN rows behind the L rows of every (b, n, h) slab, att and att_sym in sentinel storage, the workspace
    is NaN with a sentinel guard behind the elements rf_tied_logits_long_ws_elems asks for."""
    att_ld = att_ld or (L + 7) // 8 * 8
    c = A.tied_case(B, H, N, L, with_w=False, spread=spread, seed=seed, h16=h, device=DEV)
    a = (c["q"], c["k"], c["st"], None, None, c["qscale"], B, H, N, L, att_ld)
    r64, d64 = A.tied_logits(*a, dtype=F64, detail=True)
    st = A.tied_logits(*a, dtype=F32, h16=h)
    sym_ld = H + 3
    ao, zo, so = A.att_offsets(A.PAD, B, H, L, att_ld, DEV), A.att_pad_offsets(A.PAD, B, H, L, att_ld, DEV), A.sym_offsets(A.PAD, B, H, L, sym_ld, DEV)
    a0 = A.out_storage(torch.cat([ao.reshape(-1), zo.reshape(-1)]) if zo is not None else ao, h)
    s0 = A.out_storage(so, F32)
    as_, ss = a0.clone(), s0.clone()
    need = lib.rf_tied_logits_long_ws_elems(B, H, N, L)
    splits = ops._tied_long_splits(N, B, H, L)   # (the Python mirror ops.tied_logits_long sizes its workspace with)
    assert need == splits * B * H * L * 256 * nkb(L) > 0
    ws = torch.full((need + 64,), float("nan"), device=DEV)
    ws[need:] = SENTINEL
    q, k, att, sym = P(c["q"], A.PAD), P(c["k"], A.PAD), P(as_, A.PAD), P(ss, A.PAD)
    if entry == "long":
        rc = lib.rf_tied_logits_long(q, k, i4(c["st"]), c["qscale"], att, att_ld, sym, sym_ld, B, H, N, L, 32, P(ws), need, ops.stream())
    else:
        assert att_ld == L
        rc = lib.rf_tied_logits(q, k, i4(c["st"]), None, None, c["qscale"], att, sym, sym_ld, B, H, N, L, 32, P(ws), need, ops.stream())
    assert rc == 0, rc
    code = 220 + 2 * (nkb(L) - 1)
    assert lib.rf_attn_last_route() == code, (lib.rf_attn_last_route(), code)
    torch.cuda.synchronize()
    name = f"tied_logits_long/{entry}/B{B}H{H}N{N}L{L}/ld{att_ld}/spread{spread}"
    # rows >= L of att do not exist, nothing behind the last row or in front of the first was written, the pad columns hold +0
    A.assert_untouched(a0, as_, ao, zero_off=zo, what=name)
    A.assert_untouched(s0, ss, so, what=name)
    assert (ws[need:] == SENTINEL).all(), (name, "the workspace was written past rf_tied_logits_long_ws_elems")
    att_v, sym_v = as_[ao], ss[so]
    extra = A.tied_logits_extra(d64, N)
    A.check(name, att_v, r64, st, extra, route=code, build=dn(h))
    # every row sums to 1 within the rounding of its entries to the 16-bit type (half a unit in the last place each: 2^-8 relative
    # with bfloat16's 8 significant bits, 2^-11 with fp16's 11, and 2^-25 absolute below fp16's normal range), the softmax
    # allowance of the oracle and the roundings of the fp32 row sum
    half = 2.0 ** -8 if h == torch.bfloat16 else 2.0 ** -11
    tol = half * r64.sum(-1) + (L * 2.0 ** -25 if h == torch.float16 else 0.0) + extra.sum(-1) + (L + 4) * 2.0 ** -24
    assert ((att_v.to(F64).sum(-1) - 1).abs() <= tol).all(), (name, (att_v.to(F64).sum(-1) - 1).abs().max().item())
    s64 = A.tied_sym(att_v)  # 0.5 * (a + b) of two stored 16-bit values is one fp32 rounding: exact
    assert torch.equal(sym_v.to(F64), A.rnd(s64, F32)), (name, "att_sym is not the symmetrisation of the stored att")
    assert torch.equal(sym_v, sym_v.transpose(1, 2)), (name, "att_sym is not bitwise symmetric")
    return as_, ss


# one residue either side of every 128-row and 256-column block edge, and one short of the top
LONG_LENGTHS = [257, 300, 383, 385, 511, 513, 641, 767, 769, 1000, 1023]


@pytest.mark.parametrize("L", LONG_LENGTHS)
def test_tied_logits_long(h16, L):
    """B = 1, H = 1, N = 4 (one range of four MSA rows: the ring's prologue runs past the range)"""
    run_long(1, 1, 4, L, h16, spread=30.0 if L % 2 else 4.0, seed=L)


def test_tied_logits_long_four_ranges(h16):
    """B = 2, H = 3, N = 136: four ranges of 34 MSA rows, summed by the softmax kernel"""
    run_long(2, 3, 136, 300, h16, spread=4.0, seed=136)


def test_tied_logits_long_other_leading_dimension(h16):
    """att_ld = L + 16: inside the key tiles at L = 400, above them at L = 1016 (the zero fill runs past the last tile)"""
    run_long(1, 1, 4, 400, h16, att_ld=416, spread=4.0, seed=5)
    run_long(1, 2, 8, 1016, h16, att_ld=1032, spread=30.0, seed=6)


@pytest.mark.parametrize("L", [512, 768, 1024])
def test_whole_tiles_are_rf_tied_logits_bit_for_bit(h16, L):
    a_long, s_long = run_long(1, 1, 4, L, h16, att_ld=L, seed=L)
    a_old, s_old = run_long(1, 1, 4, L, h16, att_ld=L, seed=L, entry="plain")
    assert torch.equal(bits(a_long), bits(a_old)) and torch.equal(s_long.cpu().view(torch.int32), s_old.cpu().view(torch.int32))


def test_refusals(h16):
    """values only: every call returns before a launch, the buffers stay zero"""
    z = torch.zeros(1 << 22, device=DEV, dtype=h16)
    zf = torch.zeros(1 << 22, device=DEV)
    s = ops.stream()

    def long(L, N=8, ld=None, ws=zf, ws_elems=None):
        ld = ld or (L + 7) // 8 * 8
        st = (N * L * 32, L * 32, L * 32, 32)
        return lib.rf_tied_logits_long(P(z), P(z), i4(st), 1.0, P(z), ld, None, 0, 1, 1, N, L, 32, P(ws) if ws is not None else None,
                                       zf.numel() if ws_elems is None else ws_elems, s)
    assert long(256) == EINVAL and long(1025) == EINVAL
    assert long(300, N=7) == EINVAL and long(300, N=132) == EINVAL
    need = lib.rf_tied_logits_long_ws_elems(1, 1, 8, 300)
    assert need == 2 * 300 * 512   # (six tiles: the eight MSA rows go in two ranges of four)
    assert long(300, ws=None, ws_elems=0) == EINVAL and long(300, ws_elems=need - 1) == EINVAL
    assert long(300, ld=300) == EALIGN and long(300, ld=308) == EALIGN
    assert long(300, ld=296) == EINVAL
    for bad in ((1, 1, 7, 300), (1, 1, 132, 300), (1, 1, 8, 256), (1, 1, 8, 1025)):
        assert lib.rf_tied_logits_long_ws_elems(*bad) == 0
    # the old entry points keep their lengths
    st = (8 * 300 * 32, 300 * 32, 300 * 32, 32)
    assert lib.rf_tied_logits_ld(P(z), P(z), i4(st), None, None, 1.0, P(z), 304, None, 0, 1, 1, 8, 300, 32, P(zf), zf.numel(), s) == EINVAL
    assert lib.rf_tied_logits(P(z), P(z), i4(st), None, None, 1.0, P(z), None, 0, 1, 1, 8, 300, 32, P(zf), zf.numel(), s) == EINVAL
    torch.cuda.synchronize()
    assert not z.any() and not zf.any()


# ================================================================================================ rf_poswise_collapsed
NTS = (1, 2, 3, 4, 5, 6, 7, 8, 12, 16)


def poswise_code(N):
    return 260 + min(t for t in NTS if 16 * t >= N)


def run_poswise(B, N, L, D, H, spread, h, seed=0):
    """tests/test_attn_bound_gpu.py::run_poswise with the route code of a depth that fills no tile"""
    scale = spread / 5.0 / D ** 0.5
    xo = A.strided_offsets(A.PAD, (N * L * D, L * D, D, 1), (B, N, L, D), DEV)
    uo = A.strided_offsets(A.PAD, (L * H * D, H * D, D, 1), (B, L, H, D), DEV)
    xn = A.image_storage(xo, A.randn((B, N, L, D), seed, DEV), h)
    u = A.image_storage(uo, A.randn((B, L, H, D), seed + 1, DEV), h)
    a = (xn, u, B, N, L, D, H, scale)
    r64, d64 = A.poswise_collapsed(*a, dtype=F64, detail=True)
    st = A.poswise_collapsed(*a, dtype=F32, h16=h)
    wo = A.poswise_offsets(A.PAD, B, H, N, L, DEV)
    w0 = A.out_storage(wo, F32)
    ws = w0.clone()
    assert lib.rf_poswise_collapsed(P(xn, A.PAD), P(u, A.PAD), P(ws, A.PAD), B, N, L, D, H, scale, ops.stream()) == 0
    code = poswise_code(N)
    assert lib.rf_attn_last_route() == code, (lib.rf_attn_last_route(), code)
    torch.cuda.synchronize()
    A.assert_untouched(w0, ws, wo)  # the sentinel in front of and behind w
    got, extra = ws[wo], A.poswise_extra(d64, D)
    # (one MSA row: the softmax over n is 1 whatever the logit, every correct evaluation stores exactly 1: declared exact, as
    # run_logits declares L == 1)
    A.check(f"poswise_collapsed/B{B}N{N}L{L}D{D}H{H}/spread{spread}", got, r64, st, extra, route=code, build=dn(h), exact=N == 1)
    assert ((got.to(F64).sum(-1) - 1).abs() <= extra.sum(-1) + (N + 4) * 2.0 ** -24).all()
    return ws


@pytest.mark.parametrize("N", [1, 15, 17, 37, 100, 129, 200, 255])
def test_poswise_collapsed_any_depth(h16, N):
    i = 0
    for H in (1, 12):
        for D in (32, 384):
            for L in (1, 5):
                run_poswise(2, N, L, D, H, 30.0 if i % 2 else 4.0, h16, seed=N + H + i)
                i += 1


@pytest.mark.parametrize("N", [48, 256])
def test_poswise_collapsed_whole_tiles_are_unchanged(h16, N):
    """a depth that fills its tiles: the code of test_attn_bound_gpu (260 + N / 16, the aligned instantiation: a tail launch of
    the same tile count exists only below 16 NT) and the same bits on a copy of the inputs"""
    assert poswise_code(N) == A.poswise_code(N)
    first = run_poswise(2, N, 5, 384, 12, 4.0, h16, seed=N)
    again = run_poswise(2, N, 5, 384, 12, 4.0, h16, seed=N)
    assert torch.equal(first.view(torch.int32), again.view(torch.int32))
    z, zf = torch.zeros(1 << 16, device=DEV, dtype=h16), torch.zeros(1 << 16, device=DEV)
    assert lib.rf_poswise_collapsed(P(z), P(z), P(zf), 1, 257, 4, 32, 4, 1.0, ops.stream()) == EINVAL
    assert lib.rf_poswise_collapsed(P(z), P(z), P(zf), 1, 0, 4, 32, 4, 1.0, ops.stream()) == EINVAL
    torch.cuda.synchronize()
    assert not zf.any()


# ================================================================================================ the module
MODES = [(torch.float32, 2e-4), (torch.bfloat16, 4e-2), (torch.float16, 6e-3)]  # tests/test_tied_ragged_gpu.py
DM, NH = 384, 12


@pytest.fixture(params=MODES, ids=["fp32", "bf16", "fp16"])
def mode(request):
    R.set_compute_dtype(request.param[0])
    return request.param


@pytest.fixture
def routes(monkeypatch):
    """launch counters: the head-major core, the general path's softmax, both long-row launches"""
    calls = {"fused": [], "general": [], "long": ops.COUNTERS["tied_logits_long"], "long_ragged": []}
    fused, general, ragged = ops.tied_attention, ops.tied_softmax, ops.tied_logits_long

    def counted_fused(q, k, v, out, att, **kw):
        calls["fused"].append((q.shape[3], att.shape[3]))
        return fused(q, k, v, out, att, **kw)

    def counted_general(logits, att, *a, **kw):
        calls["general"].append((logits.shape[2], att.shape[3]))
        return general(logits, att, *a, **kw)

    def counted_ragged(q, k, att, *a, **kw):
        calls["long_ragged"].append((q.shape[3], att.shape[3]))
        return ragged(q, k, att, *a, **kw)
    monkeypatch.setattr(ops, "tied_attention", counted_fused)
    monkeypatch.setattr(ops, "tied_softmax", counted_general)
    monkeypatch.setattr(ops, "tied_logits_long", counted_ragged)
    return calls


def rel(a, b):
    """max |a-b| / max |b|  (tests/test_tied_ragged_gpu.py)"""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-20)).item()


@functools.lru_cache(maxsize=None)
def case(N, Lr):
    """module (CPU, seeded), input and the oracle's outputs: one reference per shape, shared by the modes and never modified"""
    torch.manual_seed(11)
    m = R.SoftTiedAttentionOverResidues(DM, NH, 0.0, return_att=True)
    x = torch.randn(1, N, Lr, DM, generator=torch.Generator().manual_seed(N + Lr))
    P_ = {"m." + k: v.detach().float() for k, v in m.state_dict().items()}
    ro, ra = O.soft_tied_attention(P_, "m", x, NH)
    return m, x, ro, ra


def run_module(N, Lr, mode, routes):
    m, x, ro, ra = case(N, Lr)
    m = m.to(DEV)
    try:
        out, att = m(x.to(DEV))
        torch.cuda.synchronize()
    finally:
        m.to("cpu")
    e_o, e_a = rel(out, ro), rel(att, ra)
    print(f"soft tied N={N} L={Lr} {mode[0]}: out {e_o:.3e} att {e_a:.3e} routes {routes}")
    assert e_o < mode[1] and e_a < mode[1]
    assert torch.equal(att, att.transpose(1, 2))
    return out, att


@pytest.mark.parametrize("N,Lr", [(64, 257), (64, 300)])
def test_soft_tied_attention_long_ragged(N, Lr, mode, routes):
    run_module(N, Lr, mode, routes)
    ld = ops.tied_ld(Lr)
    if mode[0] == torch.float32:
        assert routes["long_ragged"] == [] and routes["general"] == [(Lr, Lr)] and routes["fused"] == [], routes
    else:
        assert routes["long_ragged"] == [(Lr, ld)] and ops.COUNTERS["tied_logits_long"] - routes["long"] == 1, routes
        assert routes["general"] == [] and routes["fused"] == [], routes
        assert lib.rf_attn_last_route() == 222


@pytest.mark.parametrize("N,Lr", [(100, 137), (100, 256)])
def test_soft_tied_attention_any_depth(N, Lr, mode, routes):
    run_module(N, Lr, mode, routes)
    if mode[0] == torch.float32:
        assert routes["fused"] == [] and routes["general"] == [(Lr, Lr)], routes
    else:
        assert routes["fused"] == [(Lr, ops.tied_ld(Lr))] and routes["general"] == [] and routes["long_ragged"] == [], routes
        # 137: weights in the one-pass kernel's 192-row tail form; 256: folded into q, the contraction-split form; then attention . V
        assert lib.rf_attn_last_route() == (211245 if Lr == 137 else 220246), lib.rf_attn_last_route()


def test_switch_restores_the_general_route(mode, routes):
    RT.tied_long_ragged = False
    run_module(64, 300, mode, routes)
    ld = ops.tied_ld(300) if ops.is_h16(mode[0]) else 300
    assert routes["long_ragged"] == [] and routes["fused"] == [] and routes["general"] == [(300, ld)], routes
    assert ops.COUNTERS["tied_logits_long"] == routes["long"]


# ------------------------------------------------------------------------------------------------ one recorded backward
BWD = (1, 64, 257, DM, NH)


@functools.lru_cache(maxsize=None)
def bwd_setup(p_dropout=0.0):
    B, N, L, D, H = BWD
    torch.manual_seed(100 + L + D)
    mod = G.randomize(R.SoftTiedAttentionOverResidues(D, H, p_dropout=p_dropout, return_att=True), 200 + L,
                      lambda name: "fn.0.weight" in name)
    g = G.gen(300 + L + N)
    return mod, torch.randn(B, N, L, D, generator=g), torch.randn(B, N, L, D, generator=g), torch.randn(B, L, L, H, generator=g)


def loss_of(o, w_o, w_a):
    """sum(out * w_o) + sum(att * w_a)"""
    return (o[0] * w_o).sum() + (o[1] * w_a).sum()


def module_grads(mod, x, w_o, w_a):
    before = ops.COUNTERS["tied_logits_long"]

    def loss(o):
        assert ops.COUNTERS["tied_logits_long"] - before == 1 and lib.rf_attn_last_route() == 222   # recorded on the long route
        assert o[0].requires_grad and o[1].requires_grad
        return loss_of(o, w_o.to(DEV), w_a.to(DEV))
    return {k: t.clone() for k, t in G.grads_of(mod, {"x": x}, loss)[0].items()}


def test_recorded_backward_against_float64_autograd():
    """enable_backward(), (N, L) = (64, 257), bf16: x and every parameter gradient under the ceiling of tests/grad_oracle.py
    (relative L2 of a whole gradient, 5e-2 in bfloat16; no kinks); both to_k biases exactly zero, as in
    tests/test_tied_backward_gpu.py"""
    R.set_compute_dtype(torch.bfloat16)
    mod, x, w_o, w_a = bwd_setup()
    ref, _ = G.oracle_grads(lambda P_, xd: O.soft_tied_attention(P_, "m", xd, BWD[4]), G.state(mod), {"x": x},
                            lambda o: loss_of(o, w_o.double(), w_a.double()))
    with G.recording(mod):
        got = module_grads(mod, x, w_o, w_a)
    zero = {k: 1e-10 * ref[k.replace("bias", "weight")].norm() for k in ("m.to_k.bias", "m.poswise_weight.to_k.0.bias")}
    G.compare(got, ref, torch.bfloat16, f"{BWD} long ragged", zero=zero, unreached_zero=True)


def test_recorded_backward_in_train_mode_repeats_bitwise():
    """train() with the position weights' dropout on: the same seed gives the same bits twice"""
    R.set_compute_dtype(torch.bfloat16)
    mod, x, w_o, w_a = bwd_setup(0.1)
    mod = mod.to(DEV).train().enable_backward()
    try:
        res = []
        for _ in range(2):
            R.manual_seed(77)
            got = module_grads(mod, x, w_o, w_a)
            res.append([got[k] for k in sorted(got)])
        mod.eval()
        with torch.no_grad():
            plain = mod(x.to(DEV))[0]
            mod.train()
            R.manual_seed(77)
            assert not torch.equal(mod(x.to(DEV))[0], plain)   # the dropouts act
    finally:
        mod.eval().enable_backward(False)
        mod.to("cpu")
    assert all(torch.isfinite(t).all() for t in res[0])
    assert all(torch.equal(a, b) for a, b in zip(*res))


# ------------------------------------------------------------------------------------------------ graph capture
def test_long_ragged_forward_captures_into_a_graph():
    """nothing on the route reads back from the device: the bf16 forward at (64, 300) captures and replays bitwise"""
    R.set_compute_dtype(torch.bfloat16)
    m, x, _, _ = case(64, 300)
    m = m.to(DEV)
    try:
        xd = x.to(DEV)
        before = ops.COUNTERS["tied_logits_long"]
        eager = [t.clone() for t in m(xd)]
        assert ops.COUNTERS["tied_logits_long"] - before == 1
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(xd)                                  # weight copies are prepared outside the capture
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):
                out = m(xd)
        torch.cuda.current_stream().wait_stream(side)
        for _ in range(2):
            for t in out:
                t.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(out, eager))
    finally:
        m.to("cpu")
