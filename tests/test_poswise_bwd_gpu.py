"""rf_poswise_bwd (csrc/backward.hip): the backward of rf_poswise, alone (the direct form, any number of heads) and with
rf_weighted_msa_sum fused behind it (the collapsed one-head form of the structure track's node input).

The kernel is held against float64 autograd of a restatement of the forward on the operands as rounded, by the yardstick rule
of tests/grad_oracle.py.  The units are 2^-24 for the fp32 dq0 and an fp32 dk, the 16-bit type's unit for a 16-bit dk.  A row is
one (b, l) -- one softmax over the MSA depth each (for dk: every n of it); the margin is 4 because a depth of two or three
averages no rounding error away.  A row whose float64 gradient is exactly zero (all of dq0 at N = 1) must be exactly zero.

RF_INITIAL_COORD_BACKWARD_ERRORS=FILE: the measured errors are also merged into that JSON file (key "kernel_errors")."""
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
# (form, (B, N, L, H, dlen)): the direct form k = to_k(x) per head; the collapsed form k = x itself, one head, fused with ds.
# N = 1 (dlogit = 0), 2 and 3 (the cancellation), 65 (a second trip of a wave's lanes), 130 x 3 (N * H crosses 256 threads);
# dlen 384 is the model's width; the last two of each form have a dlen that is no multiple of 8: the scalar path.
SHAPES = [("direct", (2, 1, 5, 3, 8)), ("direct", (1, 2, 7, 1, 8)), ("direct", (2, 3, 5, 12, 32)), ("direct", (1, 65, 4, 4, 24)),
          ("direct", (1, 130, 3, 3, 16)), ("direct", (1, 5, 3, 2, 12)),
          ("fused", (2, 1, 5, 1, 16)), ("fused", (1, 3, 7, 1, 24)), ("fused", (1, 65, 4, 1, 384)), ("fused", (1, 130, 3, 1, 40)),
          ("fused", (1, 4, 3, 1, 20))]
# (id, library's 16-bit type, operand dtype): fp32 operands, and the 16-bit type of each build
OPERANDS = [("fp32", torch.bfloat16, torch.float32), ("bf16", torch.bfloat16, torch.bfloat16),
            ("fp16", torch.float16, torch.float16)]
OP_DTYPE = {o[0]: o[2] for o in OPERANDS}
NAMES = ("dq0", "dk")
RECORDS = []
# dk's storage type -> the units of (dq0, dk); a row is every n of one (b, l)
UNITS = {dt: {"dq0": G.UNIT[torch.float32], "dk": G.UNIT[dt]} for dt in G.UNIT}
HELD = dict(rows="bl", records=RECORDS)
_restore_mode = G.restore_mode()
_write_records = G.records_fixture("RF_INITIAL_COORD_BACKWARD_ERRORS", RECORDS,
                                   "max(torch float32 autograd vs float64, unit of the storage type)")


@pytest.fixture(params=OPERANDS, ids=[o[0] for o in OPERANDS])
def operand(request):
    R.set_compute_dtype(request.param[1])
    return request.param


# ---- the forward, restated (any floating type; differentiable) -------------------------------------------------------------------
def weights(q0, k, H, scale, keep=None, p=0.0):
    """q0 [B, L, H*dlen], k [B, N, L, H*dlen] -> w [B, N, H, L] = softmax over n; keep [B, N, H, L]: the dropout's keep map"""
    B, N, L, HD = k.shape
    logit = torch.einsum("blhc,bnlhc->bnhl", q0.view(B, L, H, HD // H), k.view(B, N, L, H, HD // H)) * scale
    w = logit.softmax(1)
    return w if keep is None else w * (keep.to(w.dtype) / (1.0 - p))


def loss(q0, k, H, scale, dw, ds, keep=None, p=0.0):
    """sum(w * dw) + sum(s * ds), s = sum_n w_n k_n (one head); either gradient may be None"""
    w = weights(q0, k, H, scale, keep, p)
    out = 0.0
    if dw is not None:
        out = out + (w * dw).sum()
    if ds is not None:
        out = out + (torch.einsum("bnl,bnlc->blc", w[:, :, 0], k) * ds).sum()
    return out


def autograd(c, dtype, keep=None, p=0.0):
    q0, k = (c[n].detach().cpu().to(dtype).clone().requires_grad_() for n in ("q0", "k"))
    dw, ds = (None if c[n] is None else c[n].detach().cpu().to(dtype) for n in ("dw", "ds"))
    loss(q0, k, c["H"], c["scale"], dw, ds, None if keep is None else keep.cpu(), p).backward()
    return {"dq0": q0.grad, "dk": k.grad}


@functools.lru_cache(maxsize=None)
def case(form, shape, op_id):
    """One set of operands per (form, shape, operand type), shared by the tests below and left unchanged.  Direct: q0 and k of
    the operand type, dw, and a dk of the operand type (what PositionWiseWeightFactor asks for).  Fused: q0 fp32, k of the
    operand type, ds, and an fp32 dk (what the node input asks for)."""
    B, N, L, H, dlen = shape
    dt = OP_DTYPE[op_id]
    g_ = G.gen(3000 + 7 * N + dlen)
    k = torch.randn(B, N, L, H * dlen, generator=g_).to(dt).to(DEV)
    q0 = torch.randn(B, L, H * dlen, generator=g_).to(dt if form == "direct" else torch.float32).to(DEV)
    dw = torch.randn(B, N, H, L, generator=g_).to(DEV) if form == "direct" else None
    ds = torch.randn(B, L, dlen, generator=g_).to(DEV) if form == "fused" else None
    return dict(q0=q0, k=k, dw=dw, ds=ds, H=H, scale=dlen ** -0.5, dlen=dlen, dk_dtype=dt if form == "direct" else torch.float32)


@functools.lru_cache(maxsize=None)
def refs(form, shape, op_id, drop=None):
    """(float64 autograd, float32 autograd) of the restatement on the case's operands; drop = (p, seed, offset): with the keep
    map rf_dropout draws over the contiguous [B, N, H, L] weights"""
    c = case(form, shape, op_id)
    keep, p = None, 0.0
    if drop is not None:
        p, keep = drop[0], keep_map(shape, drop)
    return autograd(c, torch.float64, keep, p), autograd(c, torch.float32, keep, p)


def keep_map(shape, drop):
    B, N, L, H, _ = shape
    ones = torch.ones(B, N, H, L, device=DEV)
    return ops.dropout(ones, drop[0], drop[1], drop[2], out=torch.empty_like(ones)) != 0


def run_bwd(c, dropout=None, **over):
    t = dict(c, **over)
    B, N, L, HD = t["k"].shape
    H, dlen = t["H"], t["dlen"]
    dq0, dk = ops.poswise_bwd(t["q0"], HD, t["k"], HD, 0, dlen if H > 1 else 0, dlen, B, N, L, H, t["scale"], dw=t["dw"], ds=t["ds"],
                              dk_dtype=t["dk_dtype"], dropout=dropout)
    return {"dq0": dq0, "dk": dk}


# ---- 1. the kernel against float64 autograd ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,shape", SHAPES, ids=[f"{f}-{s}" for f, s in SHAPES])
def test_kernel_against_float64_autograd(form, shape, operand):
    c = case(form, shape, operand[0])
    ref64, ref32 = refs(form, shape, operand[0])
    got = run_bwd(c)
    assert got["dq0"].dtype == torch.float32 and got["dk"].dtype == c["dk_dtype"]
    assert got["dq0"].shape == c["q0"].shape and got["dk"].shape == c["k"].shape
    assert G.held(got, ref64, ref32, f"{operand[0]} {form} {shape}", UNITS[c["dk_dtype"]], **HELD)
    if shape[1] > 1:   # the check has teeth: the weights' gradient with two MSA rows swapped must fail it
        swap = {n: None if c[n] is None else c[n].flip(1 if n == "dw" else 2).contiguous() for n in ("dw", "ds")}
        assert not G.held(run_bwd(c, **swap), ref64, ref32, f"{operand[0]} {form} {shape} (flipped gradient: must fail)",
                          UNITS[c["dk_dtype"]], **HELD)
        del RECORDS[-len(NAMES):]


# ---- 2. exact facts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,shape", [SHAPES[0], SHAPES[6]], ids=["direct", "fused"])
def test_depth_one_gives_exact_zeros(form, shape, operand):
    """N = 1: the softmax is the constant 1, so dlogit = 0: dq0 is exactly zero, dk is the weighted-sum term alone"""
    c = case(form, shape, operand[0])
    got = run_bwd(c)
    assert (got["dq0"] == 0).all()
    if form == "direct":
        assert (got["dk"] == 0).all()
    else:
        assert torch.equal(got["dk"], c["ds"][:, None].expand_as(got["dk"]))     # dk_0 = w_0 ds with w_0 = 1 (an fp32 dk)
    p = 0.25
    keep = keep_map(shape, (p, 7, 3))
    dropped = run_bwd(c, dropout=(p, 7, 3))
    assert (dropped["dq0"] == 0).all()
    if form == "fused":   # wd = keep / (1 - p)
        want = c["ds"][:, None] * (keep[:, :, 0, :, None].float() / (1.0 - p))
        torch.testing.assert_close(dropped["dk"], want, rtol=2 * G.UNIT[torch.float32], atol=0.0)
        assert (dropped["dk"][~keep[:, :, 0]] == 0).all()


def test_both_gradients_add_and_strided_addressing_gives_the_same_bits(operand):
    """dw and ds in one call (fp32 autograd of the sum as the yardstick), and the direct form read from / written into the
    columns of wider buffers, like the fused q | k | poswise-k projection of the attention layers"""
    dt = operand[2]
    shape = (1, 3, 7, 1, 24)
    c = dict(case("fused", shape, operand[0]))
    c["dw"] = torch.randn(1, 3, 1, 7, generator=G.gen(5)).to(DEV)
    got = run_bwd(c)
    assert G.held(got, autograd(c, torch.float64), autograd(c, torch.float32), f"{operand[0]} fused+dw {shape}", UNITS[c["dk_dtype"]],
                  **HELD)
    del RECORDS[-len(NAMES):]
    B, N, L, H, dlen = shape = (2, 3, 5, 12, 32)
    c = case("direct", shape, operand[0])
    plain = run_bwd(c)
    HD, ld, col0 = H * dlen, 3 * H * dlen + 8, 2 * H * dlen
    kbuf = torch.full((B, N, L, ld), float("nan"), device=DEV).to(dt)
    kbuf[..., col0:col0 + HD] = c["k"]
    dkbuf = torch.full((B, N, L, ld), 7.0, device=DEV).to(dt)
    dq0, dk = ops.poswise_bwd(c["q0"], HD, kbuf, ld, col0, dlen, dlen, B, N, L, H, c["scale"], dw=c["dw"], dk=dkbuf, dk_ld=ld,
                              dk_col0=8, dk_hs=dlen)
    assert dk is dkbuf and torch.equal(dq0, plain["dq0"]) and torch.equal(dkbuf[..., 8:8 + HD], plain["dk"])
    assert (dkbuf[..., :8] == 7).all() and (dkbuf[..., 8 + HD:] == 7).all()
    # a column offset that is no multiple of 8 takes the scalar path: the same sums in the same order
    dkbuf2 = torch.full((B, N, L, ld), 7.0, device=DEV).to(dt)
    kbuf2 = torch.full((B, N, L, ld), float("nan"), device=DEV).to(dt)
    kbuf2[..., 3:3 + HD] = c["k"]
    dq0b, _ = ops.poswise_bwd(c["q0"], HD, kbuf2, ld, 3, dlen, dlen, B, N, L, H, c["scale"], dw=c["dw"], dk=dkbuf2, dk_ld=ld,
                              dk_col0=5, dk_hs=dlen)
    ref64, ref32 = refs("direct", shape, operand[0])
    assert G.held({"dq0": dq0b, "dk": dkbuf2[..., 5:5 + HD]}, ref64, ref32, f"{operand[0]} direct {shape} (scalar path)", UNITS[dt],
                  **HELD)
    del RECORDS[-len(NAMES):]
    assert (dkbuf2[..., :5] == 7).all() and (dkbuf2[..., 5 + HD:] == 7).all()


# ---- 3. dropout replay ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,shape", [SHAPES[2], SHAPES[7]], ids=["direct", "fused"])
def test_dropout_replay(form, shape, operand):
    drop = (0.25, 1234, 5)
    c = case(form, shape, operand[0])
    ref64, ref32 = refs(form, shape, operand[0], drop)
    got = run_bwd(c, dropout=drop)
    assert G.held(got, ref64, ref32, f"{operand[0]} {form} {shape} dropout={drop[0]}", UNITS[c["dk_dtype"]], **HELD)
    again = run_bwd(c, dropout=drop)
    other = run_bwd(c, dropout=(drop[0], drop[1] + 1, drop[2]))
    for n in NAMES:
        assert torch.equal(got[n], again[n]) and not torch.equal(got[n], other[n]), n
    plain64, _ = refs(form, shape, operand[0])      # and the dropout matters: the reference without it is far away
    assert G.errors(got["dk"], plain64["dk"], "bl")[0] > 0.1


# ---- 4. determinism and refusals -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,shape", [SHAPES[4], SHAPES[8]], ids=["direct", "fused"])
def test_two_runs_give_the_same_bits(form, shape):
    R.set_compute_dtype(torch.bfloat16)
    c = case(form, shape, "bf16")
    a, b = run_bwd(c, dropout=(0.25, 3, 1)), run_bwd(c, dropout=(0.25, 3, 1))
    assert all(torch.equal(a[n], b[n]) for n in a)
    a, b = run_bwd(c), run_bwd(c)
    assert all(torch.equal(a[n], b[n]) for n in a)


def test_entry_point_refuses_before_a_launch():
    R.set_compute_dtype(torch.bfloat16)
    B, N, L, H, dlen = 1, 3, 4, 2, 8
    q0 = torch.zeros(B, L, H * dlen, device=DEV)
    k = torch.zeros(B, N, L, H * dlen, device=DEV)
    dw = torch.zeros(B, N, H, L, device=DEV)
    ds = torch.zeros(B, L, dlen, device=DEV)
    dq0, dk = torch.zeros_like(q0), torch.zeros_like(k)
    p_ = ops.ptr

    def call(q0_=q0, k_=k, dw_=dw, ds_=None, dq0_=dq0, dk_=dk, N_=N, H_=H, p=0.0):
        return _lib.lib.rf_poswise_bwd(p_(q0_), _lib.RF_F32, H * dlen, p_(k_), _lib.RF_F32, H * dlen, 0, dlen, dlen, p_(dw_), p_(ds_),
                                       dlen, p_(dq0_), p_(dk_), _lib.RF_F32, H * dlen, 0, dlen, B, N_, L, H_, 0.3, p, 0, 0,
                                       ops.stream())

    assert call() == 0
    assert call(p=0.5) == 0
    assert call(H_=1, ds_=ds) == 0               # one head with both gradients
    for name in ("q0_", "k_", "dq0_", "dk_"):    # RF_EINVAL: a NULL tensor
        assert call(**{name: None}) == -1, name
    assert call(dw_=None) == -1                  # neither dw nor ds
    assert call(ds_=ds) == -1                    # the collapsed form fused with ds takes one head: dk would sum over heads
    assert call(p=1.0) == -1 and call(p=-0.1) == -1
    assert call(N_=3969) == -1                 # (2 * N * H + 512) * 4 bytes of LDS > 64 KB at H = 2: refused, nothing launched
    assert call(N_=7937, H_=1) == -1
    torch.cuda.synchronize()
    with pytest.raises(ValueError):              # the wrapper's own checks: k too small for the addressing
        ops.poswise_bwd(q0, H * dlen, k, H * dlen, 8, dlen, dlen, B, N, L, H, 0.3, dw=dw)
    with pytest.raises(ValueError):
        ops.poswise_bwd(q0, H * dlen, k, H * dlen, 0, dlen, dlen, B, N, L, H, 0.3, dw=dw[:, :2])
    with pytest.raises(ValueError):
        ops.poswise_bwd(q0, H * dlen, k, H * dlen, 0, dlen, dlen, B, N, L, H, 0.3, dw=dw, ds=ds)
