"""The machinery every HIP backward pass shares (opt-in per module: RecordingModule.enable_backward in model.py).

A module gains a backward pass with four things on its class, next to the forward they differentiate:
  * its kernel sequence (`run` / `attend` / `apply_residual`) takes `tape=`: a dict that receives what the backward needs --
    same launches, same numbers as the plain call;
  * `_backward(tape, g) -> (dx, {param: grad})` on the module's own layout;
  * `_record(x, tape)`, the forward() body with the boundary layout conversion, and `_backward_from_autograd`, its mirror image
    (RecordingModule's default serves a module whose boundary needs none);
  * `_backward_children()`: the sub-modules enable_backward() switches along.
A module of several inputs (OuterProductMean) sets `_rf_n_inputs = n` on its class: `_record(x_1 .. x_n, tape)` (an optional
input may be None), and `_backward_from_autograd` receives a tuple of n "wanted" flags and returns a tuple of n gradients.
_RecordedFn below is the one autograd Function of the package: it ties them to torch.autograd."""
import math

import torch

from . import ops
from .ops import F32
from .runtime import RT, T, dropout_, _f


def _recording(mod):
    """record an autograd graph only when the module opted in AND grad mode is on (requires_grad alone never switches it on)"""
    return getattr(mod, "_rf_backward", False) and torch.is_grad_enabled()


def _check_backward_call(mod, tape, row_group, *channels):
    """In front of every kernel sequence that takes a tape.  The backward pass does not cover row-sharded calls: refused when one
    is being recorded (a tape) or would be (the module opted in and grad mode is on).  With a tape, the channel counts the
    backward kernels contract over must be multiples of 8."""
    if row_group is not None and (tape is not None or _recording(mod)):
        raise NotImplementedError(f"{type(mod).__name__}: the backward pass does not support row-sharded calls (row_group)")
    for c in channels if tape is not None else ():
        if c % 8:
            raise ValueError(f"{type(mod).__name__}: the backward pass needs channel counts that are multiples of 8, got {c}")


def _copy(t):
    return ops.axpby(t, 1.0, None, 0.0, torch.empty(t.shape, device=t.device, dtype=t.dtype))


def _dropout_rec(t, p):
    """dropout_(t, p) returning what the backward replays: (p, seed, offset), or None when nothing was dropped."""
    if p is None or p <= 0.0 or t.numel() == 0:
        return None
    rec = (p, RT.train_seed, RT.train_offset)
    dropout_(t, p)
    return rec


def _replay_dropout(g, rec):
    """multiply g by the forward's mask / (1 - p) (rf_dropout with the recorded seed and offset), in place"""
    if rec is None:
        return g
    p, seed, off = rec
    return ops.fill(g, 0.0) if p >= 1.0 else ops.dropout(g, p, seed, off)


def _grad_scale(gs):
    """Power of two that brings max |g| into [1, 2) in the fp16 mode, whose 16-bit gradient operands would underflow for small
    losses; 1 in the other modes.  Exact: every backward step is linear in the gradient, the scale is undone in fp32."""
    if RT.dtype != torch.float16:
        return 1.0
    m = ops.absmax(gs)
    if not math.isfinite(m) or m == 0.0:
        return 1.0
    return 2.0 ** max(-100, min(100, -math.floor(math.log2(m))))


def _scaled_copy(g, s):
    """fresh contiguous fp32 s * g (autograd may hand in expanded or non-contiguous gradients)"""
    g = g.float().contiguous()
    return ops.axpby(g, s, None, 0.0, torch.empty(g.shape, device=g.device, dtype=F32))


def _unscale(ts, s):
    if s != 1.0:
        for t in ts:
            if t is not None:
                ops.axpby(t, 1.0 / s, None, 0.0, t)


def _conv_weight_grad(dw, w):
    """fp32 [Co, 9 * Ci] gradient in the forward's [co][tap][ci] layout -> a contiguous [Co, Ci, 3, 3] like the weight"""
    Co, Ci = w.shape[0], w.shape[1]
    out = torch.empty(Co, Ci, 3, 3, device=dw.device, dtype=F32)
    ops.copy(dw.view(Co, 9, Ci).transpose(1, 2), out.view(Co, Ci, 9))
    return out


def _param_grads(mod, grads, s):
    ps = list(mod.parameters())
    out = [grads.get(p) for p in ps]
    _unscale(out, s)
    return tuple(out)


class _RecordedFn(torch.autograd.Function):
    """forward() of a module that opted in, under grad mode: apply(mod, x, *mod.parameters()), or with mod._rf_n_inputs = n
    apply(mod, x_1 .. x_n, *mod.parameters()).  Runs mod._record into a fresh tape; the backward hands the output gradients to
    mod._backward_from_autograd and spreads its {param: grad} over the parameters (and its n input gradients over the inputs).  fp16 power-of-two scale (_grad_scale): chosen here over the raw output gradients, applied and taken off dx by
    the adaptor, taken off the parameter gradients here -- unless the module scales its own operands (_rf_scales_own_grads)."""

    @staticmethod
    def forward(ctx, mod, *args):
        tape = {}
        out = mod._record(*args[:mod._rf_n_inputs], tape)
        ctx.mod, ctx.tape = mod, tape
        return out

    @staticmethod
    def backward(ctx, *gs):
        mod = ctx.mod
        s = 1.0 if mod._rf_scales_own_grads else _grad_scale([g.float().contiguous() for g in gs])
        n = mod._rf_n_inputs
        want = ctx.needs_input_grad[1:1 + n]
        dxs, grads = mod._backward_from_autograd(ctx.tape, gs, s, want[0] if n == 1 else want)
        ctx.tape = None
        dxs = (dxs,) if n == 1 else tuple(dxs)
        return (None,) + tuple(d if w else None for d, w in zip(dxs, want)) + _param_grads(mod, grads, s)


def _pre_norm_residual_bwd(g, sub_backward, sub_tape, x_in, lnm, grads):
    """Backward of x += f(LayerNorm(x)) for the gradient g of the updated x (fp32, accumulated in place): f's backward runs on
    a copy of g brought to the fp16 mode's power-of-two scale, the LayerNorm's on the saved fp32 input."""
    s = _grad_scale([g])
    dxn, gr = sub_backward(sub_tape, _scaled_copy(g, s))
    dx, dgamma, dbeta = ops.layernorm_bwd(x_in, dxn, _f(lnm.weight), eps=lnm.eps)
    gr.update({lnm.weight: dgamma, lnm.bias: dbeta})
    _unscale([dx] + list(gr.values()), s)
    ops.axpby(g, 1.0, dx, 1.0, g)
    grads.update(gr)


def conv_input_grad_weight(w):
    """[Co, Ci, k, k] kernel of a stride-1 "same" convolution -> [Ci, Co, k, k]: its input gradient (any dilation) is the same
    convolution of the output gradient with the kernel rotated 180 degrees and its in / out channels swapped."""
    return w.flip(-1, -2).transpose(0, 1)


def conv3x3_input_grad(mod, key, conv, dy, dilation, residual=None):
    """Input gradient of conv3x3 on the forward's implicit-GEMM engine (rf_gemm conv mode, conv288 at C = 288) with the repacked
    kernel: fp32 NHWC (+ residual, in place when given).  The 16-bit modes write the 16-bit type (what the 288-channel engine
    writes) and widen it; the fp32 mode writes fp32 with the exact fp32 kernel."""
    B, Hh, Ww, Co = dy.shape
    Ci = conv.weight.shape[1]
    wk = mod.cached(("conv_input_grad", key), lambda: conv_input_grad_weight(conv.weight.detach()).permute(0, 2, 3, 1)
                    .reshape(Ci, 9 * Co).to(T()).contiguous())
    if T() == F32:
        out = residual if residual is not None else torch.empty(B, Hh, Ww, Ci, device=dy.device, dtype=F32)
        return ops.gemm(dy, wk, out, B * Hh * Ww, Ci, 9 * Co, conv=(B, Hh, Ww, Co, dilation), residual=residual, exact=True)
    o16 = torch.empty(B, Hh, Ww, Ci, device=dy.device, dtype=T())
    ops.gemm(dy, wk, o16, B * Hh * Ww, Ci, 9 * Co, conv=(B, Hh, Ww, Co, dilation))
    if residual is not None:
        return ops.axpby(residual, 1.0, o16, 1.0, residual)
    return ops.axpby(o16, 1.0, None, 0.0, torch.empty(o16.shape, device=dy.device, dtype=F32))
