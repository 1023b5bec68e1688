"""rf_embedding_bwd and rf_pair_axis_sums (csrc/backward.hip): the two kernels the backward of MsaEmbedding and PairEmbedding
adds, in both builds.

Each output is held against float64 autograd of a torch restatement (a gather, i.e. index_add backwards, and broadcast sums) on
the same operands, by the yardstick rule of tests/grad_oracle.py, with 2^-24, the rounding unit of the fp32 outputs.  A row is the
last dimension: one table row, one (b, i) channel row.  Every run goes through sentinel-filled outputs with a tail, and two
runs must give the same bits.

RF_EMBEDDING_BACKWARD_ERRORS=FILE: the measured errors are also merged into that JSON file (key "kernel_errors")."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import grad_oracle as G  # noqa: E402
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import _lib, ops  # noqa: E402

DEV = "cuda"
# rf_embedding_bwd (B, N, L, D, V).  One row (dq[1] and all but one table row exactly zero); D no multiple of a wave; the
# model's width on six channel tiles with one token withheld and the values 0 and V - 1 forced in (350 rows: the second stage
# adds exactly one partial); a five-row table; a table of 64 rows, most of them unused (one wave per block); 2080 rows (the
# second stage adds three partials of four waves); and a table of 40 rows (two waves per block, two partials).
EMB_SHAPES = [(1, 1, 1, 8, 21), (2, 3, 13, 40, 21), (1, 5, 70, 384, 21), (3, 2, 37, 32, 5), (1, 2, 9, 16, 64), (2, 8, 130, 32, 21),
              (1, 4, 150, 24, 40)]
WITHHELD = {(1, 5, 70, 384, 21): 7}
DROP_SHAPES = [(2, 3, 13, 40, 21), (2, 8, 130, 32, 21)]
DROP = (0.3, 1234, 77)   # (p, seed, offset)
# rf_pair_axis_sums (B, L, D).  L = 1: dsep exactly zero; L = 2; two samples with D no multiple of a wave; the model's width over
# two column tiles and five row tiles; 257: five column tiles, seventeen row tiles, the last of one row / one column.
PAIR_SHAPES = [(2, 1, 16), (1, 2, 8), (2, 13, 40), (1, 65, 288), (1, 257, 72)]
BUILDS = [("bf16-build", torch.bfloat16), ("f16-build", torch.float16)]
SENTINEL = 7.0
RECORDS = []
HELD = dict(units=G.UNIT[torch.float32], rows=1, records=RECORDS, key="out")
_restore_mode = G.restore_mode()
_write_records = G.records_fixture("RF_EMBEDDING_BACKWARD_ERRORS", RECORDS, "max(torch float32 autograd vs float64, 2^-24)")


@pytest.fixture(params=BUILDS, ids=[b[0] for b in BUILDS])
def build(request):
    """both kernels take fp32 operands and are built into both libraries"""
    R.set_compute_dtype(request.param[1])
    return request.param[0]


# ================================================================================================ rf_embedding_bwd
@functools.lru_cache(maxsize=None)
def emb_case(shape):
    """One set of operands per shape, shared and left unchanged: the tokens [B,N,L], the gradient [B,N,L,D] and the dropout
    factors keep / (1 - p) of DROP, read off ops.dropout of a tensor of ones with the same record."""
    B, N, L, D, V = shape
    g_ = G.gen(7100 + 13 * L + D + V)
    idx = torch.randint(0, V, (B, N, L), generator=g_)
    if shape in WITHHELD:
        t = WITHHELD[shape]
        idx[idx == t] = t + 1
        idx.view(-1)[0], idx.view(-1)[-1] = 0, V - 1
        assert not (idx == t).any() and (idx == 0).any() and (idx == V - 1).any()
    g = torch.randn(B, N, L, D, generator=g_)
    factor = ops.dropout(torch.ones(B, N, L, D, device=DEV), *DROP)
    assert 0.6 < (factor != 0).float().mean().item() < 0.8 or factor.numel() < 64
    return dict(idx=idx.to(DEV), g=g.to(DEV), factor=factor)


def emb_autograd(c, V, dtype, dropped):
    """sum((table[idx] * factor + query[n > 0]) * g) differentiated by torch: (d table [V,D], d query [2,D])"""
    idx, g = c["idx"].cpu(), c["g"].cpu().to(dtype)
    B, N, L, D = g.shape
    table = torch.zeros(V, D, dtype=dtype, requires_grad=True)
    query = torch.zeros(2, D, dtype=dtype, requires_grad=True)
    y = table[idx]
    if dropped:
        y = y * c["factor"].cpu().to(dtype)
    qidx = (torch.arange(N) > 0).long()
    ((y + query[qidx][None, :, None, :]) * g).sum().backward()
    return table.grad, query.grad


@functools.lru_cache(maxsize=None)
def emb_refs(shape, dropped):
    c = emb_case(shape)
    return emb_autograd(c, shape[4], torch.float64, dropped), emb_autograd(c, shape[4], torch.float32, dropped)


def run_embedding_bwd(c, V, drop=None, with_q=True):
    """the entry point on sentinel-filled outputs with a tail of 16 elements each; checks the tails"""
    idx, g = c["idx"], c["g"]
    B, N, L, D = g.shape
    rows = B * N * L
    dt = torch.full((V * D + 16,), SENTINEL, device=DEV)
    dq = torch.full((2 * D + 16,), SENTINEL, device=DEV) if with_q else None
    wsb = int(_lib.lib.rf_embedding_bwd_ws_bytes(rows, D, V))
    assert wsb > 0
    ws = torch.empty(wsb, device=DEV, dtype=torch.uint8)
    p, seed, off = drop or (0.0, 0, 0)
    p_ = ops.ptr
    rc = _lib.lib.rf_embedding_bwd(p_(idx), p_(g), p_(dt), p_(dq), rows, D, V, N, L, p, seed, off, p_(ws), wsb, ops.stream())
    assert rc == 0
    assert (dt[V * D:] == SENTINEL).all()
    if with_q:
        assert (dq[2 * D:] == SENTINEL).all()
        dq = dq[:2 * D].view(2, D)
    return dt[:V * D].view(V, D), dq


@pytest.mark.parametrize("shape", EMB_SHAPES, ids=str)
def test_embedding_bwd_against_float64_autograd(shape, build):
    B, N, L, D, V = shape
    c = emb_case(shape)
    (t64, q64), (t32, q32) = emb_refs(shape, False)
    dt, dq = run_embedding_bwd(c, V)
    tag = f"{build} embedding_bwd {shape}"
    ref64, ref32 = {"dtable": t64, "dq": q64}, {"dtable": t32, "dq": q32}
    assert G.held({"dtable": dt, "dq": dq}, ref64, ref32, tag, **HELD)
    used = torch.zeros(V, dtype=torch.bool)
    used[c["idx"].cpu().view(-1)] = True
    assert (dt[~used.to(DEV)] == 0).all()               # a table row whose index never occurs: exact zeros
    if shape in WITHHELD:
        assert not used[WITHHELD[shape]] and used[0] and used[V - 1]
    if N == 1:
        assert (dq[1] == 0).all()
    if B * N * L == 1:
        assert int(used.sum()) == 1 and torch.equal(dt[used.to(DEV)][0], c["g"].view(-1)) and torch.equal(dq[0], c["g"].view(-1))
    again, again_q = run_embedding_bwd(c, V)            # the same bits on a second run
    assert torch.equal(again, dt) and torch.equal(again_q, dq)
    alone, none = run_embedding_bwd(c, V, with_q=False)  # dq is optional and changes nothing
    assert none is None and torch.equal(alone, dt)
    w_dt, w_dq = ops.embedding_bwd(c["idx"], c["g"], V, query=(N, L))   # the wrapper: the same bits
    assert torch.equal(w_dt, dt) and torch.equal(w_dq, dq)
    if B * N * L > 1:   # the check has teeth: the tokens shifted by one row must fail it
        wrong, _ = run_embedding_bwd(dict(c, idx=c["idx"].view(-1).roll(1).view(B, N, L).contiguous()), V)
        assert not G.held({"dtable": wrong}, {"dtable": t64}, {"dtable": t32}, "(tokens rolled by one: must fail)", **HELD)
        del RECORDS[-1]


@pytest.mark.parametrize("shape", DROP_SHAPES, ids=str)
def test_embedding_bwd_replays_the_dropout_mask(shape, build):
    """p = 0.3 with a non-zero seed and offset: the table's gradient takes the mask, the query rows' does not"""
    B, N, L, D, V = shape
    c = emb_case(shape)
    (t64, q64), (t32, q32) = emb_refs(shape, True)
    dt, dq = run_embedding_bwd(c, V, drop=DROP)
    tag = f"{build} embedding_bwd {shape} p={DROP[0]}"
    assert G.held({"dtable": dt, "dq": dq}, {"dtable": t64, "dq": q64}, {"dtable": t32, "dq": q32}, tag, **HELD)
    plain, plain_q = run_embedding_bwd(c, V)
    assert torch.equal(dq, plain_q)                     # query_enc is added behind the dropout
    assert not G.held({"dtable": plain}, {"dtable": t64}, {"dtable": t32}, "(no mask: must fail)", **HELD)
    del RECORDS[-1]
    again, _ = run_embedding_bwd(c, V, drop=DROP)
    assert torch.equal(again, dt)
    masked = ops.dropout(c["g"].clone(), *DROP)         # the acceptable alternative of the design: a masked copy in front
    assert torch.equal(run_embedding_bwd(dict(c, g=masked), V)[0], dt)
    w_dt, w_dq = ops.embedding_bwd(c["idx"], c["g"], V, query=(N, L), drop=DROP)
    assert torch.equal(w_dt, dt) and torch.equal(w_dq, dq)


def test_embedding_bwd_serves_the_pair_side(build):
    """rows = B * L, idx = seq, N = 1: the call PairEmbedding's backward makes"""
    B, L, D, V = 2, 13, 40, 21
    g_ = G.gen(7900)
    seq, g = torch.randint(0, V, (B, L), generator=g_).to(DEV), torch.randn(B, L, D, generator=g_).to(DEV)
    want = torch.zeros(V, D, dtype=torch.float64).index_add_(0, seq.cpu().view(-1), g.cpu().double().view(-1, D))
    want32 = torch.zeros(V, D).index_add_(0, seq.cpu().view(-1), g.cpu().view(-1, D))
    dt, none = ops.embedding_bwd(seq, g, V)
    assert none is None
    assert G.held({"dtable": dt}, {"dtable": want}, {"dtable": want32}, f"{build} embedding_bwd pair side {(B, L, D, V)}", **HELD)


def test_embedding_bwd_refuses_before_a_launch(build):
    shape = (2, 3, 13, 40, 21)
    B, N, L, D, V = shape
    c = emb_case(shape)
    rows = B * N * L
    dt, dq = torch.zeros(V, D, device=DEV), torch.zeros(2, D, device=DEV)
    wsb = int(_lib.lib.rf_embedding_bwd_ws_bytes(rows, D, V))
    ws = torch.empty(wsb, device=DEV, dtype=torch.uint8)
    p_ = ops.ptr

    def call(idx_=c["idx"], g_=c["g"], dt_=dt, dq_=dq, rows_=rows, D_=D, V_=V, N_=N, L_=L, p=0.0, ws_=ws, wsb_=wsb):
        return _lib.lib.rf_embedding_bwd(p_(idx_), p_(g_), p_(dt_), p_(dq_), rows_, D_, V_, N_, L_, p, 1, 2, p_(ws_), wsb_,
                                         ops.stream())

    assert call() == 0 and call(dq_=None) == 0 and call(p=0.5) == 0
    for name in ("idx_", "g_", "dt_", "ws_"):
        assert call(**{name: None}) == -1, name           # RF_EINVAL: a NULL tensor
    for name in ("rows_", "D_", "V_", "N_", "L_"):
        assert call(**{name: 0}) == -1, name
    for p in (-0.1, 1.0, 1.5, float("nan")):
        assert call(p=p) == -1, p
    assert call(wsb_=wsb - 8) == -1                       # a workspace too small
    assert call(V_=127) == -1                             # sums beyond the LDS the kernel enables: refused, nothing launched
    assert int(_lib.lib.rf_embedding_bwd_ws_bytes(rows, D, 127)) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.embedding_bwd(c["idx"], c["g"][..., :8, :], V)
    with pytest.raises(ValueError):
        ops.embedding_bwd(c["idx"].int(), c["g"], V)
    with pytest.raises(ValueError):
        ops.embedding_bwd(c["idx"], c["g"], 127)


# ================================================================================================ rf_pair_axis_sums
@functools.lru_cache(maxsize=None)
def pair_case(shape):
    """the gradient [B,L,L,D], and residue numbers that increase strictly with random gaps of 1..40 (so that the separation is
    not log(|i - j| + 1)); sep: the forward's feature in fp32"""
    B, L, D = shape
    g_ = G.gen(8100 + 11 * L + D)
    g = torch.randn(B, L, L, D, generator=g_)
    aa_idx = torch.randint(1, 41, (B, L), generator=g_).cumsum(-1)
    sep = torch.log(((aa_idx[:, :, None] - aa_idx[:, None, :]).abs() + 1).float())
    return dict(g=g.to(DEV), aa_idx=aa_idx.to(DEV), sep=sep)


def pair_autograd(c, dtype):
    """sum((r[b,i] + c[b,j] + wsep sep[b,i,j] + bias) * g) differentiated by torch: (d r, d c, d wsep, d bias)"""
    g = c["g"].cpu().to(dtype)
    B, L, _, D = g.shape
    r, cc = (torch.zeros(B, L, D, dtype=dtype, requires_grad=True) for _ in range(2))
    wsep, bias = (torch.zeros(D, dtype=dtype, requires_grad=True) for _ in range(2))
    y = r[:, :, None, :] + cc[:, None, :, :] + wsep * c["sep"].to(dtype)[..., None] + bias
    (y * g).sum().backward()
    return r.grad, cc.grad, wsep.grad, bias.grad


@functools.lru_cache(maxsize=None)
def pair_refs(shape):
    c = pair_case(shape)
    return pair_autograd(c, torch.float64), pair_autograd(c, torch.float32)


def run_pair_axis_sums(c):
    """the entry point on sentinel-filled outputs with a tail of 16 elements each; checks the tails.  (rows, cols, dsep, dbias)"""
    g, aa_idx = c["g"], c["aa_idx"]
    B, L, _, D = g.shape
    sizes = (B * L * D, B * L * D, D, D)
    outs = [torch.full((n + 16,), SENTINEL, device=DEV) for n in sizes]
    wsb = int(_lib.lib.rf_pair_axis_sums_ws_bytes(B, L, D))
    assert wsb > 0
    ws = torch.empty(wsb, device=DEV, dtype=torch.uint8)
    p_ = ops.ptr
    rc = _lib.lib.rf_pair_axis_sums(p_(g), p_(aa_idx), *[p_(o) for o in outs], B, L, D, p_(ws), wsb, ops.stream())
    assert rc == 0
    for o, n in zip(outs, sizes):
        assert (o[n:] == SENTINEL).all()
    return outs[0][:sizes[0]].view(B, L, D), outs[1][:sizes[1]].view(B, L, D), outs[2][:D], outs[3][:D]


@pytest.mark.parametrize("shape", PAIR_SHAPES, ids=str)
def test_pair_axis_sums_against_float64_autograd(shape, build):
    B, L, D = shape
    c = pair_case(shape)
    ref64, ref32 = pair_refs(shape)
    got = run_pair_axis_sums(c)
    tag = f"{build} pair_axis_sums {shape}"
    names = ("rows", "cols", "dsep", "dbias")
    assert G.held(dict(zip(names, got)), dict(zip(names, ref64)), dict(zip(names, ref32)), tag, **HELD)
    if L == 1:
        assert (got[2] == 0).all()                        # log(1) = 0: dsep exactly zero
        assert torch.equal(got[0], c["g"].view(B, L, D)) and torch.equal(got[1], c["g"].view(B, L, D))
    assert all(torch.equal(a, b) for a, b in zip(run_pair_axis_sums(c), got))       # the same bits on a second run
    assert all(torch.equal(a, b) for a, b in zip(ops.pair_axis_sums(c["g"], c["aa_idx"]), got))   # the wrapper: the same bits
    if L > 1:   # the check has teeth: the two axes swapped must fail it
        assert not G.held({"rows": got[1]}, {"rows": ref64[0]}, {"rows": ref32[0]}, "(cols for rows: must fail)", **HELD)
        del RECORDS[-1]


def test_pair_axis_sums_leaves_its_inputs_alone_and_refuses_before_a_launch(build):
    shape = (2, 13, 40)
    B, L, D = shape
    c = pair_case(shape)
    keep = {n: c[n].clone() for n in ("g", "aa_idx")}
    run_pair_axis_sums(c)
    assert all(torch.equal(c[n], t) for n, t in keep.items())
    outs = [torch.zeros(n, device=DEV) for n in (B * L * D, B * L * D, D, D)]
    wsb = int(_lib.lib.rf_pair_axis_sums_ws_bytes(B, L, D))
    ws = torch.empty(wsb, device=DEV, dtype=torch.uint8)
    p_ = ops.ptr

    def call(g_=c["g"], a_=c["aa_idx"], r_=outs[0], c_=outs[1], s_=outs[2], b_=outs[3], B_=B, L_=L, D_=D, ws_=ws, wsb_=wsb):
        return _lib.lib.rf_pair_axis_sums(p_(g_), p_(a_), p_(r_), p_(c_), p_(s_), p_(b_), B_, L_, D_, p_(ws_), wsb_, ops.stream())

    assert call() == 0
    for name in ("g_", "a_", "r_", "c_", "s_", "b_", "ws_"):
        assert call(**{name: None}) == -1, name           # RF_EINVAL: a NULL tensor
    for name in ("B_", "L_", "D_"):
        assert call(**{name: 0}) == -1, name
    assert call(wsb_=wsb - 8) == -1                       # a workspace too small
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.pair_axis_sums(c["g"][:, :, :4], c["aa_idx"])
    with pytest.raises(ValueError):
        ops.pair_axis_sums(c["g"], c["aa_idx"][:, :4])
