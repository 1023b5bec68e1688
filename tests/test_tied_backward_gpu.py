"""Backward pass of SoftTiedAttentionOverResidues (enable_backward): the module's gradients against float64 autograd through the
CPU oracle (oracle/rf_oracle.py: soft_tied_attention) in the three compute modes and on every route of the forward, the direct
call (attend(tape=) + _backward), unchanged forward numbers, dropout replay in both mask orders, fp16 small losses, determinism
and the refusals.

The gradients are held by the ceiling-or-kink-floor rule of tests/grad_oracle.py; the function has no kinks, so no kink floor
is added.  Both to_k biases add a constant to every logit of a softmax row: exact zeros here, rounding noise in the oracle.  With
one of the two outputs out of the loss some parameters are not reached: no gradient in the oracle, exact zeros here.

Routes (model.SoftTiedAttentionOverResidues.attend): every fused route needs the 16-bit modes and d_head = 32.  d_msa 32 with
two heads (d_head 16) therefore stays on the general route (rf_gemm + rf_tied_softmax) at every length, in every mode; d_msa 64
with two heads takes the one-launch logits kernel at L = 64 and, with 16 MSA rows, the ragged head-major route at L = 40 and
100; 16384 positions of d_head 32 take the head-major route, at d_msa 384 with the position weights folded into the q
projection.  The fp32 mode takes the general route at every shape."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import grad_oracle as G  # noqa: E402
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import _lib, ops  # noqa: E402
from oracle import rf_oracle as O  # noqa: E402

DEV = "cuda"
MODES, CEIL = G.MODES, G.CEIL
LOSSES = ("both", "out", "att")
# (B, N, L, D, H).  D = 32, H = 2: L = 1, no multiple of 8 (20, 100), the ragged route's shortest chain (40) and a full tile (64),
# with 3 and 16 MSA rows and one or two samples -- the general route throughout (d_head 16)
SMALL = [(2, 3, 1, 32, 2), (1, 3, 20, 32, 2), (1, 16, 40, 32, 2), (2, 16, 64, 32, 2), (2, 3, 100, 32, 2), (1, 16, 100, 32, 2)]
# d_head 32: the one-launch logits kernel (L = 64) and the ragged head-major route (16 rows, L = 40 and 100) in the 16-bit modes
HEAD32 = [(2, 3, 64, 64, 2), (1, 16, 40, 64, 2), (1, 16, 100, 64, 2)]
WIDE = (1, 16, 64, 384, 12)          # the model's width and head count
HEAD_MAJOR = (16, 16, 64, 64, 2)     # 16384 positions: the head-major route, the weights applied inside the logits kernel
FOLD = (16, 16, 64, 384, 12)         # ... and at the model's width, folded into the q projection (ops.gemm_takes_row_scale)


CENTRED = lambda name: "fn.0.weight" in name   # noqa: E731  the 1-D parameters drawn around 1
ZERO_BIASES = ("m.to_k.bias", "m.poswise_weight.to_k.0.bias")
_restore_mode = G.restore_mode()


def loss_of(out, att, w_o, w_a, kind):
    """sum(out * w_o) + sum(att * w_a), or one of the two terms"""
    total = 0.0
    if kind in ("both", "out"):
        total = total + (out * w_o).sum()
    if kind in ("both", "att"):
        total = total + (att * w_a).sum()
    return total


@functools.lru_cache(maxsize=None)
def setup(shape, p_dropout=0.0):
    """module (fp32 weights, CPU, return_att=True), input and the two outputs' weights; shared by the modes and left unchanged"""
    B, N, L, D, H = shape
    torch.manual_seed(100 + L + D)
    mod = G.randomize(R.SoftTiedAttentionOverResidues(D, H, p_dropout=p_dropout, return_att=True), 200 + L, CENTRED)
    g = G.gen(300 + L + N)
    return mod, torch.randn(B, N, L, D, generator=g), torch.randn(B, N, L, D, generator=g), torch.randn(B, L, L, H, generator=g)


@functools.lru_cache(maxsize=None)
def reference(shape, kind):
    mod, x, w_o, w_a = setup(shape)
    H = shape[4]

    return oracle(lambda P, xd: O.soft_tied_attention(P, "m", xd, H), mod, x, w_o, w_a, kind)


def oracle(fn, mod, x, w_o, w_a, kind):
    """float64 autograd of loss_of(*fn(P, x), ..): {"x", "m." + name: gradient}"""
    return G.oracle_grads(fn, G.state(mod), {"x": x}, lambda o: loss_of(*o, w_o.double(), w_a.double(), kind))[0]


def head_major_ran():
    """rf_tied_attention(_ld) was the last attention kernel: 1000 * (one-pass logits code) + (attention . V code)"""
    code = _lib.lib.rf_attn_last_route()
    return 200 <= code // 1000 <= 215 and 240 <= code % 1000 <= 247


def module_grads(mod, x, w_o, w_a, kind, scale=1.0, route=None):
    """loss.backward() through the public forward on the device: {"x", "m." + name: gradient}"""
    def loss(o):
        if route:   # (the other routes launch no kernel that leaves a code: nothing to assert there)
            assert head_major_ran(), _lib.lib.rf_attn_last_route()
        assert o[0].requires_grad and o[1].requires_grad
        return loss_of(*o, w_o.to(DEV), w_a.to(DEV), kind)
    return G.grads_of(mod, {"x": x}, loss, scale)[0]


def compare(got, ref, dtype, tag):
    """the to_k biases: exact zeros, the oracle's own value below 1e-10 of the weight's gradient (or that weight unreached too)"""
    zero = {}
    for key in set(ZERO_BIASES) & set(ref):
        weight = ref[key.replace("bias", "weight")].norm()
        zero[key] = 1e-10 * weight if weight > 0 else float("inf")
    G.compare(got, ref, dtype, tag, zero=zero, unreached_zero=True)


def check_against_oracle(shape, dtype, kinds=LOSSES, route=None):
    R.set_compute_dtype(dtype)
    mod, x, w_o, w_a = setup(shape)
    with G.recording(mod):
        for kind in kinds:
            got = module_grads(mod, x, w_o, w_a, kind, route=route if ops.is_h16(dtype) else False)
            compare(got, reference(shape, kind), dtype, f"{shape} loss={kind}")


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_grads_against_oracle(dtype, shape):
    check_against_oracle(shape, dtype, route=False)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("shape", HEAD32, ids=str)
def test_grads_against_oracle_d_head_32(dtype, shape):
    check_against_oracle(shape, dtype, route=shape[1] == 16)


@pytest.mark.parametrize("dtype", MODES)
def test_grads_against_oracle_at_the_models_width(dtype):
    """d_msa 384, 12 heads, 1024 positions: too few for the head-major route (16384), so the one-launch logits kernel runs in
    front of the general route's attention . V"""
    check_against_oracle(WIDE, dtype, route=False)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_grads_against_oracle_on_the_head_major_route(dtype):
    check_against_oracle(HEAD_MAJOR, dtype, kinds=("both",), route=True)


def test_grads_against_oracle_with_folded_weights():
    """16384 positions at the model's width: the head-major route with w * d_head^-0.5 folded into the q projection"""
    B, N, L, D, H = FOLD
    R.set_compute_dtype(torch.bfloat16)
    assert ops.gemm_takes_row_scale(B * N * L, 3 * D, D)
    check_against_oracle(FOLD, torch.bfloat16, kinds=("both",), route=True)


# ------------------------------------------------------------------------------------------------ the direct call
@pytest.mark.parametrize("dtype", MODES)
def test_direct_call_attend_with_a_tape(dtype):
    R.set_compute_dtype(dtype)
    shape = (1, 16, 100, 64, 2)
    B, N, L, D, H = shape
    mod, x, w_o, w_a = setup(shape)
    mod = mod.to(DEV)
    try:
        xn = ops.cast(x.to(DEV), dtype)
        tape, out = {}, ops.zeros(B, N, L, D, device=DEV, dtype=torch.float32)
        att, _ = mod.attend(xn, out, True, tape=tape)
        assert tape["w_order"] == ("bhnl" if ops.is_h16(dtype) else "bnhl") and tape["drops"] == [] and tape["pw"]["drop"] is None
        dxn, grads = mod._backward(tape, w_o.to(DEV).clone(), w_a.to(DEV).clone())
        got = dict({"m." + n: grads[p] for n, p in mod.named_parameters()}, x=dxn)
        compare(got, reference(shape, "both"), dtype, f"{shape} direct")
        dxn2, grads2 = mod._backward(tape, w_o.to(DEV).clone())      # no gradient on the map
        got = dict({"m." + n: grads2[p] for n, p in mod.named_parameters()}, x=dxn2)
        compare(got, reference(shape, "out"), dtype, f"{shape} direct, out alone")
    finally:
        mod.to("cpu")


# ------------------------------------------------------------------------------------------------ forward unchanged
@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("shape", [SMALL[2], HEAD32[0], HEAD32[2], HEAD_MAJOR], ids=str)
def test_recording_forward_is_bitwise_unchanged(dtype, shape):
    R.set_compute_dtype(dtype)
    mod, x, _, _ = setup(shape)
    mod = mod.to(DEV)
    try:
        xd = x.to(DEV)
        with torch.no_grad():
            ref = mod(xd)
        plain = mod(xd)            # grad mode on, not opted in: nothing records
        assert not plain[0].requires_grad and not plain[1].requires_grad
        assert torch.equal(plain[0], ref[0]) and torch.equal(plain[1], ref[1])
        mod.enable_backward()
        out = mod(xd.clone().requires_grad_())
        if ops.is_h16(dtype) and shape in (HEAD32[2], HEAD_MAJOR):
            assert head_major_ran(), _lib.lib.rf_attn_last_route()
        assert out[0].requires_grad and out[1].requires_grad
        assert torch.equal(out[0].detach(), ref[0]) and torch.equal(out[1].detach(), ref[1])
        with torch.no_grad():      # opted in, no grad mode: nothing records either
            again = mod(xd)
        assert torch.equal(again[0], ref[0]) and torch.equal(again[1], ref[1])
    finally:
        mod.enable_backward(False)
        mod.to("cpu")


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("shape", [SMALL[2], HEAD32[2]], ids=str)
def test_recording_forward_is_bitwise_unchanged_in_train_mode(dtype, shape):
    """train() with the default dropout (0.1 on the position weights and on the output) under the same manual_seed"""
    R.set_compute_dtype(dtype)
    mod, x, _, _ = setup(shape, 0.1)
    mod = mod.to(DEV)
    try:
        mod.train()
        xd = x.to(DEV)
        with torch.no_grad():
            R.manual_seed(77)
            ref = mod(xd)
            mod.eval()
            assert not torch.equal(mod(xd)[0], ref[0])     # the dropouts act
            mod.train()
        mod.enable_backward()
        R.manual_seed(77)
        out = mod(xd.clone().requires_grad_())
        assert out[0].requires_grad
        assert torch.equal(out[0].detach(), ref[0]) and torch.equal(out[1].detach(), ref[1])
    finally:
        mod.eval().enable_backward(False)
        mod.to("cpu")


# ------------------------------------------------------------------------------------------------ training mode
def restated(P, x, H, keep_w=None, p_w=0.0, out_drops=()):
    """soft_tied_attention (oracle/rf_oracle.py) with the dropouts as given keep maps: keep_w [B,N,H,L] on the position weights,
    out_drops = ((keep [B,N,L,D], p), ..) on the projected output.  Any floating type; differentiable."""
    B, N, L, D = x.shape
    dh = D // H
    lin = lambda name, t: F.linear(t, P[f"m.{name}.weight"], P[f"m.{name}.bias"])   # noqa: E731
    heads = lambda t: t.view(B, N, L, H, dh).permute(0, 1, 3, 2, 4)   # noqa: E731  b n h l d
    q0 = lin("poswise_weight.to_q.0", x[:, :1]).view(B, 1, L, H, dh) * dh ** -0.5
    kp = lin("poswise_weight.to_k.0", x).view(B, N, L, H, dh)
    w = torch.einsum("bqlhd,bnlhd->bnhl", q0, kp).softmax(1)
    if keep_w is not None:
        w = w * (keep_w.to(w.dtype) / (1.0 - p_w))
    q, k, v = (heads(lin(nm, x)) for nm in ("to_q", "to_k", "to_v"))
    q = q * w.unsqueeze(-1) * dh ** -0.5
    att = torch.einsum("bnhid,bnhjd->bhij", q, k).softmax(-1)
    o = torch.einsum("bhij,bnhjd->bnhid", att, v).permute(0, 1, 3, 2, 4).reshape(B, N, L, D)
    out = lin("to_out", o)
    for keep, p in out_drops:
        out = out * (keep.to(out.dtype) / (1.0 - p))
    return out, ((att + att.transpose(-1, -2)) * 0.5).permute(0, 2, 3, 1)


def keep_map(shape, rec):
    """the keep map rf_dropout draws over a contiguous tensor of `shape` for the record (p, seed, offset)"""
    ones = torch.ones(shape, device=DEV)
    return (ops.dropout(ones, rec[0], rec[1], rec[2], out=torch.empty_like(ones)) != 0).cpu()


@pytest.mark.parametrize("dtype,shape,order", [(torch.float32, (1, 16, 40, 32, 2), "bnhl"), (torch.float16, (1, 16, 100, 64, 2), "bhnl")],
                         ids=["general-route", "head-major-route"])
def test_dropout_masks_are_replayed_in_the_order_the_forward_drew_them(dtype, shape, order):
    """train(), p = 0.25 on both sites.  The general route drops the position weights in [B,N,H,L] order, the fast routes in
    [B,H,N,L] order (the fp32 mode never takes a fast route, so that order is checked in the fp16 mode): the gradients agree,
    within the mode's ceiling, with float64 autograd of the forward restated with the keep maps of the tape's records laid out
    in that order -- and with the other order's map they do not."""
    R.set_compute_dtype(dtype)
    B, N, L, D, H = shape
    mod, x, w_o, w_a = setup(shape, 0.25)
    mod = mod.to(DEV)
    try:
        mod.train()
        R.manual_seed(5)
        tape, out = {}, ops.zeros(B, N, L, D, device=DEV, dtype=torch.float32)
        mod.attend(ops.cast(x.to(DEV), dtype), out, True, drops=(0.25,), tape=tape)
        assert tape["w_order"] == order and tape["pw"]["drop"] is not None and len(tape["drops"]) == 1
        dxn, grads = mod._backward(tape, w_o.to(DEV).clone(), w_a.to(DEV).clone())
        got = dict({"m." + n: grads[p] for n, p in mod.named_parameters()}, x=dxn)
        rec = tape["pw"]["drop"]
        hm = keep_map((B, H, N, L), rec).permute(0, 2, 1, 3)      # the map drawn over [B,H,N,L], as [B,N,H,L]
        nm = keep_map((B, N, H, L), rec)
        keep_w, other = (hm, nm) if order == "bhnl" else (nm, hm)
        assert 0 < (~keep_w).sum() < keep_w.numel() and not torch.equal(keep_w, other)
        out_drops = tuple((keep_map((B, N, L, D), r), r[0]) for r in tape["drops"])

        def fn(keep):
            return lambda P, xd: restated(P, xd, H, keep, rec[0], out_drops)
        ref = oracle(fn(keep_w), mod, x, w_o, w_a, "both")
        compare(got, ref, dtype, f"{shape} train, {order}")
        wrong = oracle(fn(other), mod, x, w_o, w_a, "both")
        assert G.rel(got["x"], wrong["x"]) > 10 * CEIL[dtype]
    finally:
        mod.eval()
        mod.to("cpu")


def test_dropout_replay_finite_differences():
    """train(), fp32 (the general route), p = 0.25 on both sites: central finite differences of the recorded forward under the
    same seed along a few input elements and a few weights (form and bound of
    tests/test_axial_backward_gpu.py::test_dropout_replay_finite_differences)"""
    R.set_compute_dtype(torch.float32)
    shape = (1, 3, 20, 32, 2)
    mod, x, w_o, w_a = setup(shape, 0.25)
    with G.recording(mod, train=True):
        x, w_o, w_a = (t.to(DEV) for t in (x, w_o, w_a))

        def loss(xx):
            R.manual_seed(5)
            return loss_of(*mod(xx), w_o, w_a, "both")

        with torch.no_grad():
            mod.eval()
            plain = loss(x)
            mod.train()
            assert not torch.equal(loss(x), plain)   # the dropouts act
        for p in mod.parameters():
            p.grad = None
        xg = x.clone().requires_grad_()
        loss(xg).backward()
        g = G.gen(31)
        eps = 3e-2   # (the function is smooth: the step only has to stay well above the fp32 loss noise, ~1e-5)
        v = torch.zeros(x.numel())
        v[torch.randperm(x.numel(), generator=g)[:8]] = torch.randn(8, generator=g)   # a few input elements
        v = v.view(x.shape).to(DEV)
        with torch.no_grad():
            fd = (loss(x + eps * v) - loss(x - eps * v)).item() / (2 * eps)
        an = (xg.grad * v).sum().item()
        assert abs(fd - an) <= 2e-2 * abs(an) + 1e-3, (fd, an)
        for wt in (mod.to_q.weight, mod.to_v.weight, mod.poswise_weight.to_k[0].weight, mod.to_out.bias):
            dw = torch.zeros(wt.numel())
            dw[torch.randperm(wt.numel(), generator=g)[:8]] = torch.randn(8, generator=g)   # a few weights
            dw = dw.view(wt.shape).to(DEV)
            with torch.no_grad():
                w0 = wt.clone()
                wt.copy_(w0 + eps * dw)
                lp = loss(x).item()
                wt.copy_(w0 - eps * dw)
                lm = loss(x).item()
                wt.copy_(w0)
            an_w = (wt.grad * dw).sum().item()
            assert abs((lp - lm) / (2 * eps) - an_w) <= 2e-2 * abs(an_w) + 1e-3, ((lp - lm) / (2 * eps), an_w)


# ------------------------------------------------------------------------------------------------ fp16 small losses
def test_fp16_small_loss_does_not_underflow():
    R.set_compute_dtype(torch.float16)
    shape = (1, 16, 100, 64, 2)
    mod, x, w_o, w_a = setup(shape)
    with G.recording(mod):
        res = [module_grads(mod, x, w_o, w_a, "both", scale=s) for s in (1.0, 1e-8)]
    for key, a in res[0].items():
        b = res[1][key]
        assert torch.isfinite(b).all(), key
        if key in ZERO_BIASES:
            assert (b == 0).all()
            continue
        assert b.abs().max() > 0, key
        assert G.rel(b * 1e8, a) < CEIL[torch.float16], key


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("shape", [SMALL[4], HEAD32[2]], ids=str)
def test_backward_is_deterministic(shape):
    R.set_compute_dtype(torch.bfloat16)
    mod, x, w_o, w_a = setup(shape)
    with G.recording(mod):
        res = []
        for _ in range(2):
            got = module_grads(mod, x, w_o, w_a, "both")
            res.append([got[k].clone() for k in sorted(got)])
    assert all(torch.equal(a, b) for a, b in zip(*res))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("D,H", [(36, 2), (24, 2)], ids=["d_msa-36", "d_head-12"])
def test_channel_counts_checked_while_recording(D, H):
    R.set_compute_dtype(torch.float32)
    torch.manual_seed(7)
    mod = R.SoftTiedAttentionOverResidues(D, H, p_dropout=0.0).to(DEV)
    x = torch.randn(1, 2, 8, D, generator=G.gen(7)).to(DEV)
    with torch.no_grad():
        plain = mod(x)   # fine for the forward
    mod.enable_backward()
    with pytest.raises(ValueError):
        mod(x.clone().requires_grad_())
    with pytest.raises(ValueError):
        mod.attend(x, torch.zeros_like(x), False, tape={})
    with torch.no_grad():
        assert torch.equal(mod(x), plain)


def test_a_module_that_did_not_opt_in_records_nothing():
    R.set_compute_dtype(torch.float32)
    mod, x, _, _ = setup(SMALL[1])
    mod = mod.to(DEV)
    try:
        for p in mod.parameters():
            p.grad = None
        out, att = mod(x.to(DEV).requires_grad_())
        assert not out.requires_grad and not att.requires_grad
        assert all(p.grad is None for p in mod.parameters())
        layer = R.EncoderLayer(32, 64, 2, 0.0, tied=True).to(DEV)     # the encoder layer calls attend() without a tape
        layer.attn.enable_backward()
        assert not layer(x.to(DEV).requires_grad_()).requires_grad
    finally:
        mod.to("cpu")
