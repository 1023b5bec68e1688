"""rf_tied_softmax_bwd and rf_scale_rows_bwd (csrc/backward.hip): the two kernels the backward of
SoftTiedAttentionOverResidues adds, in both builds.

Each is held against float64 autograd of a restatement of the forward on the same operands, by the yardstick rule of
tests/grad_oracle.py.  The units are 2^-24 for fp32 outputs, the 16-bit type's unit for the 16-bit copies and a 16-bit dx.  A row
is one (b, h, i) softmax row of the map, one row of rf_scale_rows_bwd's dx; dw holds one number per row, so its worst row is its
worst element.

RF_TIED_BACKWARD_ERRORS=FILE: the measured errors are also merged into that JSON file (key "kernel_errors")."""
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
# (B, H, L): L = 1 (ds exactly zero), a very short row, either side of one wave's 64 lanes, the model's head count at a length
# that is no multiple of 8 (16-bit copies at ld = 104), and a row that crosses 256 threads
SHAPES = [(2, 2, 1), (1, 3, 5), (1, 2, 63), (1, 5, 65), (1, 12, 100), (1, 2, 257)]
BUILDS = [("bf16-build", torch.bfloat16), ("f16-build", torch.float16)]
UNIT = G.UNIT
SENTINEL = 7.0
RECORDS = []
HELD = dict(rows=1, records=RECORDS, key="out")
_restore_mode = G.restore_mode()
_write_records = G.records_fixture("RF_TIED_BACKWARD_ERRORS", RECORDS,
                                   "max(torch float32 autograd vs float64, unit of the storage type)")


@pytest.fixture(params=BUILDS, ids=[b[0] for b in BUILDS])
def build(request):
    R.set_compute_dtype(request.param[1])
    return request.param[1]


# ================================================================================================ rf_tied_softmax_bwd
def softmax_loss(logits, dp, g_sym):
    """sum(p * dp) + sum(sym * g_sym): p = softmax_j(logits) [B,H,L,L], sym[b,i,j,h] = (p[b,h,i,j] + p[b,h,j,i]) / 2"""
    p = logits.softmax(-1)
    out = (p * dp).sum()
    if g_sym is not None:
        out = out + (((p + p.transpose(-1, -2)) * 0.5).permute(0, 2, 3, 1) * g_sym).sum()
    return out, p


def softmax_autograd(c, dtype):
    lg = c["logits"].detach().cpu().to(dtype).clone().requires_grad_()
    gs = None if c["g_sym"] is None else c["g_sym"].detach().cpu().to(dtype)
    out, p = softmax_loss(lg, c["dp"].detach().cpu().to(dtype), gs)
    out.backward()
    return {"ds": lg.grad, "p": p.detach()}


@functools.lru_cache(maxsize=None)
def softmax_case(shape, sym, shift=None):
    """One set of operands per (shape, with / without g_sym, shift), shared and left unchanged.  Logits are normal with a standard
    deviation of 3; shift "row": +80 on one whole row; "half": -80 on half of one row's entries."""
    B, H, L = shape
    g_ = G.gen(4000 + 13 * L + H)
    logits = torch.randn(B, H, L, L, generator=g_) * 3
    if shift == "row":
        logits[0, H - 1, L // 2] += 80.0
    if shift == "half":
        logits[0, 0, L // 3, ::2] -= 80.0
    dp = torch.randn(B, H, L, L, generator=g_)
    g_sym = torch.randn(B, L, L, H, generator=g_) if sym else None
    return dict(logits=logits.to(DEV), dp=dp.to(DEV), g_sym=None if g_sym is None else g_sym.to(DEV))


@functools.lru_cache(maxsize=None)
def softmax_refs(shape, sym, shift=None):
    c = softmax_case(shape, sym, shift)
    return softmax_autograd(c, torch.float64), softmax_autograd(c, torch.float32)


def run_softmax_bwd(c, copies=True):
    """the entry point on sentinel-filled outputs with a tail of 16 elements each; returns the outputs and checks the tails"""
    B, H, L, _ = c["logits"].shape
    ld_ = ops.tied_ld(L)
    h16 = ops.h16()
    n32, n16 = B * H * L * L, B * H * L * ld_
    ds = torch.full((n32 + 16,), SENTINEL, device=DEV)
    p16 = torch.full((n16 + 16,), SENTINEL, device=DEV).to(h16) if copies else None
    ds16 = torch.full((n16 + 16,), SENTINEL, device=DEV).to(h16) if copies else None
    p_ = ops.ptr
    rc = _lib.lib.rf_tied_softmax_bwd(p_(c["logits"]), p_(c["dp"]), p_(c["g_sym"]), p_(ds), p_(p16), p_(ds16), ld_, B, H, L,
                                      ops.stream())
    assert rc == 0
    out = {"ds": ds[:n32].view(B, H, L, L)}
    assert (ds[n32:] == SENTINEL).all()
    if copies:
        for n, t in (("p16", p16), ("ds16", ds16)):
            assert (t[n16:].float() == SENTINEL).all(), n        # nothing past the output is touched
            m = t[:n16].view(B, H, L, ld_)
            assert (m[..., L:].float() == 0).all(), n             # the pad columns are exact zeros
            out[n] = m[..., :L]
    return out


@pytest.mark.parametrize("sym", [False, True], ids=["no-g_sym", "g_sym"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_softmax_bwd_against_float64_autograd(shape, sym, build):
    c = softmax_case(shape, sym)
    ref64, ref32 = softmax_refs(shape, sym)
    got = run_softmax_bwd(c)
    refs64 = {"ds": ref64["ds"], "ds16": ref64["ds"], "p16": ref64["p"]}
    refs32 = {"ds": ref32["ds"], "ds16": ref32["ds"], "p16": ref32["p"]}
    units = {"ds": UNIT[torch.float32], "ds16": UNIT[build], "p16": UNIT[build]}
    assert G.held(got, refs64, refs32, f"{build} tied_softmax_bwd {shape} sym={sym}", units, **HELD)
    if shape[2] == 1:
        assert (got["ds"] == 0).all() and (got["ds16"].float() == 0).all() and (got["p16"].float() == 1).all()
    else:   # the check has teeth: the gradient of the transposed map must fail it
        wrong = dict(c, dp=c["dp"].transpose(-1, -2).contiguous())
        assert not G.held(run_softmax_bwd(wrong), {"ds": ref64["ds"]}, {"ds": ref32["ds"]}, "(transposed dp: must fail)", units, **HELD)
        del RECORDS[-1]
    alone = run_softmax_bwd(c, copies=False)     # without the 16-bit copies: the same fp32 bits
    assert torch.equal(alone["ds"], got["ds"])
    if sym:                                       # and the symmetrised term matters
        assert shape[2] == 1 or not torch.equal(run_softmax_bwd(dict(c, g_sym=None))["ds"], got["ds"])


@pytest.mark.parametrize("shift", ["row", "half"])
def test_softmax_bwd_shifted_rows_stay_finite(shift, build):
    shape = (1, 5, 65)
    c = softmax_case(shape, True, shift)
    ref64, ref32 = softmax_refs(shape, True, shift)
    got = run_softmax_bwd(c)
    assert all(torch.isfinite(t.float()).all() for t in got.values())
    units = {"ds": UNIT[torch.float32]}
    assert G.held(got, {"ds": ref64["ds"]}, {"ds": ref32["ds"]}, f"{build} tied_softmax_bwd {shape} shift={shift}", units, **HELD)
    # an entry whose float64 probability is below 1e-30 contributes nothing: |ds| there is below the yardstick's absolute size
    tiny = ref64["p"] < 1e-30
    if shift == "half":
        assert tiny.any()
    y_all, _ = G.errors(ref32["ds"], ref64["ds"], 1)
    floor = G.MARGIN * max(y_all, UNIT[torch.float32]) * ref64["ds"].abs().max().item()
    assert (got["ds"].cpu()[tiny].abs() <= floor).all()


def test_softmax_bwd_is_deterministic_and_refuses_before_a_launch(build):
    c = softmax_case((1, 12, 100), True)
    a, b = run_softmax_bwd(c), run_softmax_bwd(c)
    assert all(torch.equal(a[n], b[n]) for n in a)
    B, H, L = 1, 2, 5
    lg, dp, ds = (torch.zeros(B, H, L, L, device=DEV) for _ in range(3))
    c16 = torch.zeros(B, H, L, 8, device=DEV).to(ops.h16())
    p_ = ops.ptr

    def call(lg_=lg, dp_=dp, ds_=ds, p16_=None, ld_=8, L_=L):
        return _lib.lib.rf_tied_softmax_bwd(p_(lg_), p_(dp_), None, p_(ds_), p_(p16_), None, ld_, B, H, L_, ops.stream())

    assert call() == 0 and call(p16_=c16) == 0
    for name in ("lg_", "dp_", "ds_"):
        assert call(**{name: None}) == -1, name     # RF_EINVAL: a NULL tensor
    assert call(L_=0) == -1
    assert call(p16_=c16, ld_=4) == -1            # a 16-bit copy with ld < L
    assert call(p16_=c16, ld_=12) == -2           # RF_EALIGN: ld no multiple of 8
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.tied_softmax_bwd(lg, dp[:, :1])


# ================================================================================================ rf_scale_rows_bwd
# (tokens, H, D), rows = tokens * H: 1, 255 and 4099 rows of 8, 16 and 32 columns (a lane group of each size; one row, a block
# that is not full, many blocks), and two cases of several heads
SCALE_CASES = [(r, 1, d) for r in (1, 255, 4099) for d in (8, 16, 32)] + [(85, 3, 8), (37, 2, 32)]
OPERANDS = ["fp32", "h16"]


def scale_autograd(c, dtype):
    x, gy, w = (c[n].detach().cpu().to(dtype) for n in ("x", "gy", "w"))
    x, w = x.clone().requires_grad_(), w.clone().requires_grad_()
    ((c["alpha"] * w[:, :, None] * x) * gy).sum().backward()
    return {"dx": x.grad, "dw": w.grad}


@functools.lru_cache(maxsize=None)
def scale_case(tokens, H, D, dt):
    g_ = G.gen(5000 + tokens + D)
    x, gy = (torch.randn(tokens, H, D, generator=g_).to(dt).to(DEV) for _ in range(2))
    return dict(x=x, gy=gy, w=torch.randn(tokens, H, generator=g_).to(DEV), alpha=0.375)   # (a float32 number, not 1)


@pytest.mark.parametrize("operand", OPERANDS)
@pytest.mark.parametrize("case", SCALE_CASES, ids=str)
def test_scale_rows_bwd_against_float64_autograd(case, operand, build):
    tokens, H, D = case
    dt = torch.float32 if operand == "fp32" else build
    c = scale_case(tokens, H, D, dt)
    ref64, ref32 = scale_autograd(c, torch.float64), scale_autograd(c, torch.float32)
    dx, dw = ops.scale_rows_bwd(c["x"], H * D, D, c["gy"], H * D, D, c["w"].view(-1), c["alpha"], tokens, H, D)
    assert dx.dtype == dt and dw.dtype == torch.float32
    got = {"dx": dx.view(tokens, H, D), "dw": dw.view(tokens, H, 1)}
    ref64, ref32 = ({"dx": r["dx"], "dw": r["dw"].unsqueeze(-1)} for r in (ref64, ref32))
    units = {"dx": UNIT[dt], "dw": UNIT[torch.float32]}
    assert G.held(got, ref64, ref32, f"{build} scale_rows_bwd {case} {operand}", units, **HELD)
    again = ops.scale_rows_bwd(c["x"], H * D, D, c["gy"], H * D, D, c["w"].view(-1), c["alpha"], tokens, H, D)
    assert torch.equal(again[0], dx) and torch.equal(again[1], dw)
    flipped = ops.scale_rows_bwd(c["x"], H * D, D, c["gy"].flip(-1).contiguous(), H * D, D, c["w"].view(-1), c["alpha"], tokens, H, D)
    if tokens > 1:   # the check has teeth
        assert not G.held({"dx": flipped[0].view(tokens, H, D), "dw": flipped[1].view(tokens, H, 1)}, ref64, ref32,
                          "(flipped gradient: must fail)", units, **HELD)
        del RECORDS[-2:]


def test_scale_rows_bwd_walks_the_q_block_of_a_projection_buffer(build):
    """x is the q block of a [tokens, 3 D] buffer (ld = 3 D, head stride d_head), dx goes into the q block of another one: the
    same bits as the contiguous call, nothing else written"""
    tokens, H, dh = 85, 3, 8
    D = H * dh
    c = scale_case(tokens, H, dh, build)
    plain_dx, plain_dw = ops.scale_rows_bwd(c["x"], D, dh, c["gy"], D, dh, c["w"].view(-1), c["alpha"], tokens, H, dh)
    xbuf = torch.full((tokens, 3 * D), float("nan"), device=DEV).to(build)
    xbuf[:, :D] = c["x"].view(tokens, D)
    dxbuf = torch.full((tokens, 3 * D), SENTINEL, device=DEV).to(build)
    dx, dw = ops.scale_rows_bwd(xbuf, 3 * D, dh, c["gy"], D, dh, c["w"].view(-1), c["alpha"], tokens, H, dh, dx=dxbuf, dx_ld=3 * D,
                                dx_hs=dh)
    assert dx is dxbuf and torch.equal(dxbuf[:, :D], plain_dx) and torch.equal(dw, plain_dw)
    assert (dxbuf[:, D:].float() == SENTINEL).all()
    # a block further in, through the element offsets
    kbuf = torch.full((tokens, 3 * D), float("nan"), device=DEV).to(build)
    kbuf[:, D:2 * D] = c["x"].view(tokens, D)
    dxbuf2 = torch.full((tokens, 3 * D), SENTINEL, device=DEV).to(build)
    _, dw2 = ops.scale_rows_bwd(kbuf, 3 * D, dh, c["gy"], D, dh, c["w"].view(-1), c["alpha"], tokens, H, dh, dx=dxbuf2,
                                dx_ld=3 * D, dx_hs=dh, x_off=D, dx_off=2 * D)
    assert torch.equal(dxbuf2[:, 2 * D:], plain_dx) and torch.equal(dw2, plain_dw) and (dxbuf2[:, :2 * D].float() == SENTINEL).all()
    with pytest.raises(ValueError):     # the wrapper's own check: x too small for the addressing
        ops.scale_rows_bwd(c["x"], 3 * D, dh, c["gy"], D, dh, c["w"].view(-1), c["alpha"], tokens, H, dh)
    p_ = ops.ptr
    code = ops.dcode(build)

    def call(x_=c["x"], w_=c["w"], dx_=plain_dx, dw_=plain_dw, tokens_=tokens, ld_=D):
        return _lib.lib.rf_scale_rows_bwd(p_(x_), code, ld_, dh, p_(c["gy"]), code, D, dh, p_(w_), 0.375, p_(dx_), code, D, dh, p_(dw_),
                                          tokens_, H, dh, ops.stream())

    assert call() == 0 and call(dx_=None) == 0 and call(dw_=None) == 0
    assert call(x_=None) == -1 and call(w_=None) == -1 and call(dx_=None, dw_=None) == -1
    assert call(tokens_=0) == -1 and call(ld_=-1) == -1
    torch.cuda.synchronize()
