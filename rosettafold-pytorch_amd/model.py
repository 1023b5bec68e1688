"""RoseTTAFold forward path on MI355X: the reference's nn.Module call surface over librfmi.so.

Class names, constructor arguments, `state_dict()` key names and forward signatures mirror
rosettafold_pytorch/rosettafold_pytorch.py (cited per class as rf.py:LINE) so that a user of the
reference can switch packages; the arithmetic inside every forward is a sequence of HIP kernels
reached through the C ABI (include/rfmi.h).  PyTorch supplies device memory, the stream and the
parameter containers (nn.Linear / nn.LayerNorm / ... are used for their weights and default init
only -- their own forward is never called).

Inference semantics: every dropout is the identity (the reference's unregistered layer lists
ignore .eval(); here they are proper ModuleLists and their weights appear in
state_dict under `...encoder_layers.N.` / `...blocks.N.`).

Precision policy: the two residual streams (msa, pair) are fp32 in HBM; GEMM operands are the
compute dtype (bf16 by default -> v_mfma_f32_16x16x32_bf16 with fp32 accumulation, or fp32 ->
exact fp32 tiles for parity runs); LayerNorm / InstanceNorm / softmax statistics are fp32; the
SE(3) structure module is fp32 end to end, as in the reference (se3_modules.py:164).
"""
import math
from collections import namedtuple

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .ops import F32
from .runtime import RT, T, manual_seed, dropout_, _f, fresh_f32  # noqa: F401  (re-exported: model.RT is the one runtime)
from .backward import (_RecordedFn, _recording, _check_backward_call, _copy, _dropout_rec, _replay_dropout,  # noqa: F401
                       _grad_scale, _scaled_copy, _unscale, _conv_weight_grad, _param_grads, _pre_norm_residual_bwd,
                       conv_input_grad_weight, conv3x3_input_grad)

N_IDX, CA_IDX, C_IDX = 0, 1, 2  # rf.py:15
M_FEAT = 266   # performer nb_features = int(64 * ln 64)
M_PAD = 288    # padded to a multiple of 32 for the MFMA K loop
VT_ROWS = 80   # 64 value rows + the ones row (k' sums) padded to a multiple of 16
_SeqGeometry = namedtuple("_SeqGeometry", "B Ls Lo ss so RB R S W2 ctx_scale")   # PerformerSelfAttention._geometry


def set_compute_dtype(dtype):
    """Operand type of the dense contractions (accumulation, residual streams, statistics and the structure track are
    fp32 in every mode):
      torch.bfloat16  v_mfma_f32_16x16x32_bf16, librfmi.so (default: the dtype BASELINE.json quotes the metric on);
      torch.float16   v_mfma_f32_16x16x32_f16, librfmi_f16.so: same rate and bytes, 8x smaller operand rounding
                      (11 significand bits), fp16 range -- the mode that carries the whole-model parity claim at speed;
      torch.float32   fp32 operands.  With set_float32_matmul_precision("highest") (the default) exact fp32 tiles
                      (v_mfma_f32_16x16x4_f32, 1/16 of the rate): the strict oracle-parity mode.  With "high" the rf_gemm
                      contractions split each fp32 operand into two bf16 pieces and take three bf16 MFMAs per product
                      (RF_F32X3, about 2^-16 relative operand error); the structure track stays exact.
    Kernel-ready weight copies are cached per dtype, so switching back and forth costs nothing after the first forward."""
    if dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise TypeError("compute dtype must be bfloat16, float16 or float32")
    RT.dtype = dtype
    L.select_h16(L.RF_F16 if dtype == torch.float16 else L.RF_BF16)
    ops.set_split_f32(dtype == torch.float32 and RT.f32_precision == "high")


def set_float32_matmul_precision(precision):
    """Precision of the fp32 GEMMs of the float32 compute mode, named after torch.set_float32_matmul_precision:
      "highest"  exact fp32 tiles (default);
      "high"     split bf16: x = hi + lo, hi . hi + hi . lo + lo . hi in fp32 accumulators (RF_F32X3, include/rfmi.h).
    Stored in every mode, in effect only under set_compute_dtype(torch.float32): the few fp32 GEMMs of the 16-bit modes and
    the structure track (fp32 end to end by design) stay exact.  A GraphedForward captured under the other precision
    raises on replay (recapture())."""
    if precision not in ("highest", "high"):
        raise ValueError(f'float32 matmul precision must be "highest" or "high", got {precision!r}')
    RT.f32_precision = precision
    ops.set_split_f32(RT.dtype == torch.float32 and precision == "high")


def get_float32_matmul_precision():
    return RT.f32_precision


def _p(drop_module):
    """p of an nn.Dropout container (0 for anything else)."""
    return float(drop_module.p) if isinstance(drop_module, nn.Dropout) else 0.0


def add_dropped(x_res, compute, drops, recs=None):
    """x_res += dropout_{p_k}(... dropout_{p_1}(f)) for the training-mode forward: `compute(tmp)` ADDS f to the zeroed fp32 tmp
    (every producer of the forward path accumulates into a residual stream: handing it zeros yields f itself).
    recs: a list that receives each dropout's (p, seed, offset) record (the recording forward of enable_backward)."""
    tmp = ops.zeros(*x_res.shape, device=x_res.device, dtype=F32)
    compute(tmp)
    for pk in drops:
        if recs is None:
            dropout_(tmp, pk)
        else:
            recs.append(_dropout_rec(tmp, pk))
    return ops.axpby(x_res, 1.0, tmp, 1.0, x_res)


def pad8(n):
    return (n + 7) // 8 * 8


def weights_fingerprint(module):
    """Changes whenever a parameter / buffer of `module` is rebound, moved or edited in place THROUGH THE TENSOR ITSELF
    (p.copy_, nn.init.*, optimizer steps bump `_version`; `p.data = other`, `.to()` change `data_ptr`).
    NOT seen: in-place edits through the `.data` alias (`p.data.copy_(w)`, `p.data.normal_()`, EMA `p.data.lerp_`): `.data`
    is a detached tensor with a version counter of its own, and a content probe would cost a device read-back per
    forward.  After such an edit call `invalidate_weight_caches(model)` (tests/test_boundary_gpu.py shows both cases);
    `load_state_dict`, `load_reference_weights`, `load_checkpoint`, `.to()` and `set_compute_dtype` need nothing."""
    h = 0
    for t in list(module.parameters()) + list(module.buffers()):
        h = (h * 1000003 + t.data_ptr() + 7919 * t._version) & 0xFFFFFFFFFFFFFFF
    return h


def invalidate_weight_caches(module):
    """Drop every kernel-ready weight copy held below `module` (they are rebuilt on the next call)."""
    RT.cache_epoch += 1
    for m in module.modules():
        c = getattr(m, "_rfc", None)
        if isinstance(c, dict):
            c.clear()
        elif c is not None:
            object.__setattr__(m, "_rfc", None)


class RFModule(nn.Module):
    """nn.Module with a cache of kernel-ready weights (cast / concatenated / padded).  The cache is validated against the
    live parameters at every PUBLIC call (`module(...)`): internal composition goes through `.run()` / `.attend()`, so
    the check costs one pass over the parameter list per user-level call, not per kernel."""

    def __init__(self):
        super().__init__()
        # Constructed in EVAL mode (nn.Module's default is training): this build's forward is the inference path, and the
        # reference hard-codes non-zero dropout probabilities in places (rf.py:1015,1101; PairUpdateWithMsa's default) that a
        # caller passing p_dropout=0 does not reach.  model.train() switches every dropout site on (Philox masks, manual_seed).
        self.training = False
        object.__setattr__(self, "_rfc", {})
        object.__setattr__(self, "_rf_fp", None)

    def _apply(self, fn, *a, **k):
        invalidate_weight_caches(self)
        return super()._apply(fn, *a, **k)

    def _load_from_state_dict(self, *a, **k):
        self._rfc.clear()
        RT.cache_epoch += 1
        return super()._load_from_state_dict(*a, **k)

    def __call__(self, *a, **k):
        fp = weights_fingerprint(self)
        if fp != self._rf_fp:
            if self._rf_fp is not None:
                invalidate_weight_caches(self)
            object.__setattr__(self, "_rf_fp", fp)
        return super().__call__(*a, **k)

    def cached(self, key, fn):
        k = (key, RT.dtype)
        v = self._rfc.get(k)
        if v is None:
            with torch.no_grad():
                v = fn()
            self._rfc[k] = v
        return v

    # operand conditioning of an attention layer's value path (16-bit modes; csrc/condition.hip) -----------------------------------
    def value_conditioning(self, xn, to_v, to_out, lead=()):
        """The attention output o = sum_j a_ij v_j (a_i. sums to one: softmax rows, or FAVOR's ratio) is a per-sample constant
        c ~ mean_j v_j plus a part 10-30x smaller at random init, and it is the 16-bit operand of the output projection:
        rounded with the constant it was 4e-2 of the bf16 mode's 5e-2 logits gap (tools/precision_probe.py --gemm-sweep
        msa_update_using_self_att:bf16; the linear attention's context, rounded for its second GEMM, another 2e-2).  With
        mu = an estimate of mean(xn) (rf_sample_mean) and c = W_v mu + b_v:
            v - c = W_v xn - W_v mu            the value block of the projection gets the bias -W_v mu instead of b_v,
            o - c = sum_j a_ij (v_j - c)       the attention kernels run unchanged on the centred values,
            W_o (o - c) + (b_o + W_o c)        the output projection gets the bias b_o + W_o b_v + (W_o W_v) mu.
        ONE constant serves the whole batch (the identity holds for any c; the constant is dominated by biases, LayerNorm
        offsets and the mean embedding, which the samples share), so the projections stay single launches over all samples.
        Returns (fp32 [1, n_lead + d_v] bias of the projection whose output columns are [lead..., v], fp32 [1, d_out] output bias);
        `lead`: the Linear modules in front of v in a fused projection (their biases pass through)."""
        def make():
            wv, wo = to_v.weight.detach().float(), to_out.weight.detach().float()
            dev = wv.device
            bl = [(_f(m_.bias) if m_.bias is not None else torch.zeros(m_.weight.shape[0], device=dev)) for m_ in lead]
            bo = _f(to_out.bias) if to_out.bias is not None else torch.zeros(wo.shape[0], device=dev)
            if to_v.bias is not None:
                bo = bo + wo @ _f(to_v.bias)
            nl = sum(m_.weight.shape[0] for m_ in lead)
            wc = torch.cat([torch.zeros(nl, wv.shape[1], device=dev), -wv, wo @ wv]).contiguous()
            bc = torch.cat(bl + [torch.zeros(wv.shape[0], device=dev), bo]).contiguous()
            return wc, bc, nl + wv.shape[0]
        wc, bc, npre = self.cached(("vcond", len(lead)), make)
        r = ops.fold_mean(wc, ops.sample_mean(xn.view(1, -1, xn.shape[-1])), bc)
        return r[:, :npre], r[:, npre:]

    # kernel-ready views of parameter containers -------------------------------------------------
    def wt(self, key, lin, kpad=None):
        def make():
            w = lin.weight.detach().reshape(lin.weight.shape[0], -1)
            if kpad is not None and kpad != w.shape[1]:
                w = torch.cat([w, w.new_zeros(w.shape[0], kpad - w.shape[1])], 1)
            return w.to(T()).contiguous()
        return self.cached(("wt", key), make)

    def wt_input_grad(self, key, lin, npad=None):
        """W^T [K, N (zero-padded to npad)] of a Linear / 1x1 convolution in T: the B operand of its input gradient (backward)."""
        def make():
            w = lin.weight.detach().reshape(lin.weight.shape[0], -1)
            if npad is not None and npad != w.shape[0]:
                w = torch.cat([w, w.new_zeros(npad - w.shape[0], w.shape[1])], 0)
            return w.t().to(T()).contiguous()
        return self.cached(("wt_input_grad", key, npad), make)

    def wcat(self, key, lins):
        return self.cached(("wcat", key), lambda: torch.cat([l.weight.detach() for l in lins], 0).to(T()).contiguous())

    def bcat(self, key, lins):
        return self.cached(("bcat", key), lambda: torch.cat([l.bias.detach() for l in lins], 0).float().contiguous())

    def values_transposed(self, lin, xn, bias):
        """lin(xn) written key-contiguous: xn T [B,N,L,D] -> v_t T [B,N,D,L], v_t[b,n,(h,d),l] = (W xn[b,n,l] + bias)[(h,d)]
        (one GEMM per MSA row with the weight as the A operand, so the transposition costs no pass of its own): the B operand
        of the attention . V GEMMs, which contract over l.  16-bit modes: the key axis has the leading dimension
        Lp = ops.tied_ld(L) (v_t is [B,N,D,Lp]) with exact zeros in the pad columns, so that the contraction over Lp is a legal K
        of the 16-bit GEMM at any L; Lp == L, and the buffer is what it always was, when L % 8 == 0."""
        B, N, Lr, D = xn.shape
        Lp = map_ld(Lr)
        v_t = (torch.empty if Lp == Lr else ops.zeros)(B, N, D, Lp, device=xn.device, dtype=T())
        ops.gemm(self.wt("v", lin), xn, v_t, D, Lr, D, batch=(B * N, 1, 1), b_bs=(Lr * D, 0, 0),
                 c_bs=(D * Lp, 0, 0), c_row=(0, 0, Lp), bias=bias, bias_mode=L.BIAS_ROW)
        return v_t


def map_ld(Lr):
    """Leading dimension of an attention map [.., L, L] and of key-contiguous values [.., D, L] in the current compute dtype:
    L in float32, L rounded up to a multiple of 8 in the 16-bit modes (ops.tied_ld; zero pad columns on both operands)."""
    return ops.tied_ld(Lr) if ops.is_h16(T()) else Lr


class RecordingModule(RFModule):
    """An RFModule with an opt-in HIP backward pass (the protocol: backward.py).  forward() is `_record(x, None)`; once the
    module opted in and grad mode is on, it is `_record(x, tape)` inside the one autograd Function.  A module of several
    tensor inputs sets _rf_n_inputs and brings its own forward() (OuterProductMean)."""
    _rf_backward = False            # enable_backward
    _rf_n_inputs = 1                # tensor inputs of _record, each with a gradient of its own from _backward_from_autograd
    _rf_scales_own_grads = False    # True: _backward brings its own operands to the fp16 mode's scale (_RecordedFn leaves it at 1)

    def _backward_children(self):
        """the sub-modules whose backward this module's composes (enable_backward switches them along)"""
        return ()

    def enable_backward(self, mode=True):
        """Opt in to autograd: with grad mode on, forward() records and loss.backward() fills the .grad of every parameter (and
        of the input, if it requires grad) through the HIP backward kernels; in train() mode the backward replays the forward's
        dropout masks.  Stored on this module and the sub-modules its class docstring names (no global state); returns self."""
        self._rf_backward = bool(mode)
        for child in self._backward_children():
            child.enable_backward(mode)
        return self

    def _backward_from_autograd(self, tape, gs, s, want_dx):
        """gs: the output gradients as autograd hands them (any strides), s: the scale to bring them to.  Returns (the input's
        gradient with s taken off again, in the input's layout, or None; {param: grad} still times s).  This default serves a
        module whose _record converts no layout."""
        dx, grads = self._backward(tape, _scaled_copy(gs[0], s))
        _unscale([dx], s)
        return dx.view(gs[0].shape), grads

    def forward(self, x):
        if _recording(self):
            return _RecordedFn.apply(self, x, *self.parameters())
        return self._record(x, None)


class LayerNorm(nn.LayerNorm):
    """nn.LayerNorm as a parameter container (same state_dict keys); a direct call runs rf_layernorm, not ATen."""

    def forward(self, x):
        return ops.layernorm(x.contiguous(), _f(self.weight), _f(self.bias), eps=self.eps, out_dtype=F32)


class Linear(nn.Linear):
    """nn.Linear as a parameter container; a direct call runs rf_gemm in the current compute dtype (fp32 result)."""

    def forward(self, x):
        xt = ops.cast(x.contiguous(), T())
        return ops.linear(xt, ops.cast(self.weight.detach().contiguous(), T()), _f(self.bias), out_dtype=F32)


def project_into_residual(x, w, bias, x_res, next_ln, drops=(), xn_out=None, recs=None):
    """x_res += x @ w^T + bias, with the next LayerNorm when the fused epilogue applies (ops.linear_residual_ln); training mode:
    `drops` = the dropouts the reference applies to the projected tensor before the residual add (then returns None); recs: see
    add_dropped."""
    drops = tuple(d for d in drops if d and d > 0)
    if drops:
        add_dropped(x_res, lambda tmp: ops.linear(x, w, bias, out=tmp, residual=tmp), drops, recs)
        return None
    return ops.linear_residual_ln(x, w, bias, x_res, next_ln, xn_out)


def ln(mod, x, out_dtype=None, **kw):
    return ops.layernorm(x, _f(mod.weight), _f(mod.bias), eps=mod.eps, out_dtype=out_dtype or T(), **kw)


# ================================================================================================
# small building blocks
# ================================================================================================
class Residual(nn.Module):
    """rf.py:18-28: fn(x) + x (dropout is the identity at inference).  The model's own compositions fuse the residual
    add into the producing GEMM's epilogue; this forward serves a directly called / user-wrapped module."""

    def __init__(self, fn, p_dropout=None):
        super().__init__()
        self.training = False   # (eval by default, like every module of this build: RFModule.__init__)
        self.fn = fn
        self.p_dropout = p_dropout

    def forward(self, x):
        fx = self.fn(x)
        if isinstance(fx, tuple):
            raise TypeError("Residual wraps modules that return one tensor")
        if self.training and self.p_dropout:   # rf.py:25-26: dropout(fn(x)) + x
            fx = dropout_(fx.float().contiguous().clone(), self.p_dropout)
        out = torch.empty(x.shape, device=x.device, dtype=F32)
        return ops.axpby(fx.contiguous(), 1.0, x.contiguous(), 1.0, out)


class ColWise(nn.Module):
    """rf.py:31-41: fn over the sequences x[b, n, :, :] (attention along dim 2)."""

    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x):
        b, n, l, d = x.shape
        if isinstance(self.fn, PerformerSelfAttention):  # strided addressing inside the kernels: no reshape
            out = ops.zeros(b, n, l, d, device=x.device, dtype=F32)
            self.fn.attend(ops.cast(x.contiguous(), T()), out, axis=2)
            return out
        return self.fn(x.reshape(b * n, l, d)).reshape(b, n, l, -1)


class RowWise(nn.Module):
    """rf.py:44-54: fn over the sequences x[b, :, l, :] (attention along dim 1)."""

    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x):
        b, n, l, d = x.shape
        if isinstance(self.fn, PerformerSelfAttention):
            out = ops.zeros(b, n, l, d, device=x.device, dtype=F32)
            self.fn.attend(ops.cast(x.contiguous(), T()), out, axis=1)
            return out
        xt = torch.empty(b, l, n, d, device=x.device, dtype=x.dtype)
        ops.copy(x.transpose(1, 2), xt)
        y = self.fn(xt.view(b * l, n, d)).contiguous()
        do = y.shape[-1]
        out = torch.empty(b, n, l, do, device=x.device, dtype=y.dtype)
        ops.copy(y.view(b, l, n, do), out.transpose(1, 2))
        return out


class FeedForward(RecordingModule):
    """rf.py:270-281.  enable_backward(): the gradients of both Linears (and of the input)."""

    def __init__(self, d_emb, d_ff, p_dropout=0.1):
        super().__init__()
        self.net = nn.Sequential(Linear(d_emb, d_ff), nn.ReLU(), nn.Dropout(p_dropout), Linear(d_ff, d_emb))

    def apply_residual(self, xn, x_res, next_ln=None, drops=(), tape=None):
        """x_res += W2 relu(W1 xn + b1) + b2   (x_res fp32, in place).  With `next_ln` the second GEMM's epilogue also
        emits next_ln(x_res) (returned, or None when the fused form does not apply).
        Training mode (self.training): dropout on the hidden activations (rf.py:276) and, from the wrapping module, `drops` on
        the block's output before the residual add (rf.py:25-26, 330) -- two GEMMs with the hidden tensor in memory.
        tape: a dict that receives what _backward needs (the normalised input and the dropout records; same kernels, same
        numbers)."""
        ph = _p(self.net[2]) if self.training else 0.0
        drops = tuple(d for d in drops if d and d > 0)
        _check_backward_call(self, tape, None, xn.shape[-1], self.net[0].out_features)
        if tape is not None:
            tape.update(xn=xn, hdrop=None, drops=[])
        if ph > 0 or drops:
            w1, b1, w2, b2 = self.wt("w1", self.net[0]), _f(self.net[0].bias), self.wt("w2", self.net[3]), _f(self.net[3].bias)
            h = ops.linear(xn, w1, b1, act=L.ACT_RELU)
            if tape is not None:
                tape["hdrop"] = _dropout_rec(h, ph)
            else:
                dropout_(h, ph)
            add_dropped(x_res, lambda tmp: ops.linear(h, w2, b2, out=tmp, residual=tmp), drops,
                        tape["drops"] if tape is not None else None)
            return None
        if ops.ffn_fused_applies(xn, x_res, self.net[0].in_features, self.net[0].out_features):
            # one launch, hidden activations on chip (csrc/ffn.hip); the weights are packed once per module
            wp = self.cached("ffn_packed", lambda: ops.ffn_pack(self.net[0].weight, self.net[3].weight, T()))
            return ops.ffn_fused(xn, wp, _f(self.net[0].bias), _f(self.net[3].bias), x_res, next_ln)
        w1, b1, w2, b2 = self.wt("w1", self.net[0]), _f(self.net[0].bias), self.wt("w2", self.net[3]), _f(self.net[3].bias)
        h = ops.linear(xn, w1, b1, act=L.ACT_RELU)
        return ops.linear_residual_ln(h, w2, b2, x_res, next_ln)

    def _backward(self, tape, g):
        """g: fp32 gradient of the block's output (overwritten).  The hidden pre-activation is recomputed from the saved input
        (the fused forward never writes it).  Returns (fp32 gradient of xn, {param: grad})."""
        xn = tape["xn"]
        D = xn.shape[-1]
        R = xn.numel() // D
        l1, l2 = self.net[0], self.net[3]
        for rec in tape["drops"]:
            _replay_dropout(g, rec)
        x2 = xn.reshape(R, D)
        g_t = ops.cast(g.reshape(R, D), T())
        hpre = ops.linear(x2, self.wt("w1", l1), _f(l1.bias), out_dtype=F32)
        h = ops.linear(x2, self.wt("w1", l1), _f(l1.bias), act=L.ACT_RELU)
        _replay_dropout(h, tape["hdrop"])
        dw2, db2 = ops.conv_wgrad(g_t, h, 1, bias=True)
        gh = ops.linear(g_t, self.wt_input_grad("w2", l2), None, out_dtype=F32, exact=True)
        dh = ops.relu_dropout_bwd(gh, hpre, T(), tape["hdrop"])
        dw1, db1 = ops.conv_wgrad(dh, x2, 1, bias=True)
        dxn = ops.linear(dh, self.wt_input_grad("w1", l1), None, out_dtype=F32, exact=True)
        return dxn.view(xn.shape), {l1.weight: dw1, l1.bias: db1, l2.weight: dw2, l2.bias: db2}

    def _record(self, x, tape):
        xn = ops.cast(x.contiguous(), T())
        out = ops.zeros(*x.shape, device=x.device, dtype=F32)
        self.apply_residual(xn, out, tape=tape)
        return out


def sinusoid_table(dim, max_len):
    """rf.py:63-68 (host-side constant table)."""
    pe = torch.zeros(max_len, dim)
    denom = torch.exp(math.log(10000.0) * torch.arange(0, dim, 2) / dim)
    pos = torch.arange(0, max_len).view(-1, 1)
    pe[:, 0::2] = torch.sin(pos / denom)
    pe[:, 1::2] = torch.cos(pos / denom)
    return pe


def check_index_range(msa, seq, aa_idx, d_input, max_len):
    """The reference raises IndexError from nn.Embedding / table indexing (rf.py:73,98,115-119,155) for a token outside
    [0, d_input) or a residue index outside [0, max_len); the kernels index unchecked, so the wrappers validate first
    (one small launch + one 12-byte read-back).  Returns whether aa_idx is strictly increasing inside every sample."""
    bad_tok, bad_idx, not_mono = ops.check_inputs(msa, seq, aa_idx, d_input, max_len)
    if bad_tok:
        raise IndexError(f"token index out of range [0, {d_input})")
    if bad_idx:
        raise IndexError(f"aa_idx out of range [0, {max_len}) (max_len of the positional-encoding table)")
    return not not_mono


class SinusoidalPositionalEncoding(RFModule):
    """rf.py:57-76."""

    def __init__(self, dim, max_len, p_dropout=0.1):
        super().__init__()
        self.dim, self.max_len = dim, max_len
        self.p_dropout = p_dropout
        self.register_buffer("pos_enc", sinusoid_table(dim, max_len), persistent=False)

    def forward(self, x, aa_idx):
        """x [B,N,L,dim] + pos_enc[aa_idx] broadcast over N (rf.py:72-76; dropout: training mode only)."""
        aa_idx = aa_idx.to(x.device).contiguous()
        check_index_range(None, None, aa_idx, 1, self.max_len)
        y = ops.add_pos_enc(x.float().contiguous(), aa_idx, self.pos_enc, two_d=False)
        return dropout_(y, self.p_dropout) if self.training else y


class SinusoidalPositionalEncoding2D(RFModule):
    """rf.py:79-103."""

    def __init__(self, dim, max_len, p_dropout=0.1):
        super().__init__()
        self.max_len = max_len
        self.register_buffer("pos_enc", sinusoid_table(dim // 2, max_len), persistent=False)

    def forward(self, x, aa_idx):
        """x [B,L,L,dim] + [pos_enc[idx_i] | pos_enc[idx_j]] (rf.py:95-103)."""
        aa_idx = aa_idx.to(x.device).contiguous()
        check_index_range(None, None, aa_idx, 1, self.max_len)
        return ops.add_pos_enc(x.float().contiguous(), aa_idx, self.pos_enc, two_d=True)


def _f32_gradient(g):
    """the output gradient autograd hands in, as a contiguous fp32 tensor (itself when it already is one)"""
    return g if g.dtype == F32 and g.is_contiguous() else g.float().contiguous()


class MsaEmbedding(RecordingModule):
    """rf.py:106-120.  enable_backward(): with grad mode on, forward(x, aa_idx) records, and loss.backward() fills the .grad of
    to_embedding and query_enc through one rf_embedding_bwd call (include/rfmi.h) over the [B, N, L, d_msa] gradient; the two
    integer inputs carry no gradient and the positional table is a buffer.  In train() mode the backward replays the dropout of
    the positional-encoding site inside that kernel; query_enc is added behind the dropout and takes the unmasked gradient.
    Everything is fp32 in every compute mode: no channel count is restricted and nothing needs the fp16 mode's scale.
    RoseTTAFold._trunk calls run() without a tape and never records here."""
    _rf_n_inputs = 2   # x, aa_idx (integers: no gradient)
    _rf_scales_own_grads = True   # (there is nothing to scale: no 16-bit operand anywhere)

    def __init__(self, d_input=21, d_msa=384, max_len=260, p_pe_drop=0.1):
        super().__init__()
        self.to_embedding = nn.Embedding(d_input, d_msa)
        self.pos_enc = SinusoidalPositionalEncoding(d_msa, max_len, p_pe_drop)
        self.query_enc = nn.Embedding(2, d_msa)

    def forward(self, x, aa_idx):
        check_index_range(x.contiguous(), None, aa_idx.contiguous(), self.to_embedding.num_embeddings, self.pos_enc.max_len)
        if _recording(self):
            return _RecordedFn.apply(self, x, aa_idx, *self.parameters())
        return self.run(x, aa_idx)

    def run(self, x, aa_idx, tape=None):
        """(indices already validated)  tape: a dict that receives what _backward needs (the tokens and the dropout record; same
        kernels, same numbers)."""
        emb, pe, qe = _f(self.to_embedding.weight), self.pos_enc.pos_enc, _f(self.query_enc.weight)
        pd = self.pos_enc.p_dropout if self.training else 0.0
        x = x.contiguous()
        rec = None
        if pd and pd > 0:
            # rf.py:114-120: dropout(emb[msa] + pe[aa_idx]) + query_enc -- the dropout sits between the two additions
            y = ops.msa_embed(x, aa_idx.contiguous(), emb, pe, ops.zeros(*qe.shape, device=qe.device, dtype=F32))
            rec = _dropout_rec(y, pd)
            yq = ops.msa_embed(x, aa_idx.contiguous(), ops.zeros(*emb.shape, device=emb.device, dtype=F32),
                               ops.zeros(*pe.shape, device=pe.device, dtype=F32), qe)
            y = ops.axpby(y, 1.0, yq, 1.0, y)
        else:
            y = ops.msa_embed(x, aa_idx.contiguous(), emb, pe, qe)
        if tape is not None:
            tape.update(x=x, drop=rec)
        return y

    def _record(self, x, aa_idx, tape):
        return self.run(x, aa_idx, tape=tape)

    def _backward(self, tape, g):
        """g: contiguous fp32 [B, N, L, d_msa] gradient of the output (read once).  Returns {param: grad}: d to_embedding from the
        masked gradient keyed by the token, d query_enc from the unmasked one split first row / other rows."""
        x, rec = tape["x"], tape["drop"]
        _, N, Lr = x.shape
        V = self.to_embedding.num_embeddings
        dropped_all = rec is not None and rec[0] >= 1.0   # (dropout_ zeroes the tensor at p >= 1: no mask to replay)
        dt, dq = ops.embedding_bwd(x, g, V, query=(N, Lr), drop=None if dropped_all else rec)
        if dropped_all:
            ops.fill(dt, 0.0)
        return {self.to_embedding.weight: dt, self.query_enc.weight: dq}

    def _backward_from_autograd(self, tape, gs, s, want):
        return (None, None), self._backward(tape, _f32_gradient(gs[0]))


class PairEmbedding(RecordingModule):
    """rf.py:123-181.  The (d_pair+1 [+d_template]) -> d_pair Linear is split by input block: the two sequence-embedding
    blocks fold into two 21-row tables, the separation column into one vector (rf_pair_embed), and with use_template
    the LayerNorm'ed template block (rf.py:141-143,161-169) is one rf_gemm accumulated onto that result.
    enable_backward(): with grad mode on, forward(seq, aa_idx, template) records, and loss.backward() fills the .grad of
    embed_seq, proj and ln_template and of template where it requires grad (seq and aa_idx carry none; template may be None).
    The backward sums the [B, L, L, d_pair] gradient over each picture axis (rf_pair_axis_sums), keys the two sums by the residue
    type into the gradients of the two folded tables (rf_embedding_bwd) and unfolds them through the cached tables in exact fp32
    in every compute mode.  Only the template branch follows the compute mode (16-bit operands, the fp16 mode's scale), and only
    it needs d_pair and d_template to be multiples of 8 while recording.  RoseTTAFold._trunk calls run() without a tape and
    never records here."""
    _rf_n_inputs = 3   # seq, aa_idx (integers: no gradient), template (may be None)
    _rf_scales_own_grads = True   # the template branch alone carries 16-bit gradient operands: scaled in _backward

    def __init__(self, d_input=21, d_pair=288, max_len=260, p_pe_drop=0.1, use_template=False, d_template=64):
        super().__init__()
        self.half_d_pair = d_pair // 2
        self.embed_seq = nn.Embedding(d_input, self.half_d_pair)
        self.pos_enc = SinusoidalPositionalEncoding2D(d_pair, max_len, p_pe_drop)
        self.use_template = use_template
        if use_template:
            self.ln_template = LayerNorm(d_template)
            self.proj = Linear(d_pair + d_template + 1, d_pair)
        else:
            self.proj = Linear(d_pair + 1, d_pair)

    def forward(self, seq, aa_idx, template=None):
        if not self.use_template and template is not None:
            raise ValueError(f"[{self.__class__.__name__}]: template is not None but use_template is False")
        if self.use_template and template is None:
            # the reference fails inside nn.LayerNorm(None) (rf.py:166); same exception type, clearer text
            raise TypeError(f"[{self.__class__.__name__}]: use_template is True but no template was given")
        check_index_range(None, seq.contiguous(), aa_idx.contiguous(), self.embed_seq.num_embeddings, self.pos_enc.max_len)
        if _recording(self):
            return _RecordedFn.apply(self, seq, aa_idx, template, *self.parameters())
        return self.run(seq, aa_idx, template)

    def run(self, seq, aa_idx, template=None, tape=None):
        """(indices already validated)  tape: a dict that receives what _backward needs (the two index tensors, the fp32 template
        and its 16-bit LayerNorm; same kernels, same numbers)."""
        h = self.half_d_pair
        if self.use_template:
            _check_backward_call(self, tape, None, self.proj.weight.shape[0], self.ln_template.weight.shape[0])

        def tables():
            e = self.embed_seq.weight.detach().float().contiguous()
            w = self.proj.weight.detach().float()
            tl = ops.linear(e, w[:, :h].contiguous(), None)
            tr = ops.linear(e, w[:, h:2 * h].contiguous(), None)
            return tl, tr, w[:, 2 * h].contiguous()

        tl, tr, wsep = self.cached("tables", tables)
        seq, aa_idx = seq.contiguous(), aa_idx.contiguous()
        x = ops.pair_embed(seq, aa_idx, tl, tr, wsep, _f(self.proj.bias), self.pos_enc.pos_enc)
        if tape is not None:
            tape.update(seq=seq, aa_idx=aa_idx)
        if self.use_template:
            B, Lr = seq.shape
            if tuple(template.shape[:3]) != (B, Lr, Lr) or template.shape[-1] != self.ln_template.weight.shape[0]:
                raise ValueError(f"[{self.__class__.__name__}]: template must be [B, L, L, {self.ln_template.weight.shape[0]}]")
            wt = self.cached("wtempl", lambda: self.proj.weight.detach()[:, 2 * h + 1:].to(T()).contiguous())
            t32 = template.float().contiguous()
            tn = ln(self.ln_template, t32)
            ops.linear(tn, wt, None, out=x, residual=x)  # x += LayerNorm(template) @ W_template^T (fp32, in place)
            if tape is not None:
                tape.update(template=t32, tn=tn)
        return x

    def _record(self, seq, aa_idx, template, tape):
        return self.run(seq, aa_idx, template, tape=tape)

    def _backward(self, tape, g, want_template=True):
        """g: contiguous fp32 [B, L, L, d_pair] gradient of the output (read only).  Returns (fp32 d template or None,
        {param: grad}), nothing scaled.  With E = embed_seq.weight [V, h], W = proj.weight and the forward's tables tl = E W_l^T
        (indexed by seq[j]) and tr = E W_r^T (indexed by seq[i]), W_l = W[:, :h], W_r = W[:, h:2h]:
            rows = sum_j g, cols = sum_i g, dsep, dbias                          rf_pair_axis_sums (g read once)
            d tl = cols keyed by seq[b, j],   d tr = rows keyed by seq[b, i]     rf_embedding_bwd on [B*L, d_pair]
            dE = d tl W_l + d tr W_r,  dW_l = d tl^T E,  dW_r = d tr^T E         exact fp32 rf_gemm in every mode
            dW[:, 2h] = dsep,  d bias = dbias
        and with use_template, on s g in the compute type (s: the fp16 mode's power-of-two scale, taken off in fp32):
            dW[:, 2h+1:] = g^T LN(template)                                      rf_conv_wgrad (the forward's 16-bit LN output)
            d tn = g W_t,   d template, d gamma, d beta = LayerNorm backward     rf_gemm, rf_layernorm_bwd"""
        seq, aa_idx = tape["seq"], tape["aa_idx"]
        h, dev = self.half_d_pair, g.device
        V = self.embed_seq.num_embeddings
        D, K = self.proj.weight.shape
        rows, cols, dsep, dbias = ops.pair_axis_sums(g, aa_idx)
        dtl, _ = ops.embedding_bwd(seq, cols, V)
        dtr, _ = ops.embedding_bwd(seq, rows, V)
        e = self.embed_seq.weight.detach().float().contiguous()
        w = self.proj.weight.detach().float()
        e_t = e.t().contiguous()
        dW = torch.empty(D, K, device=dev, dtype=F32)
        dE = None
        for col0, dtab in ((0, dtl), (h, dtr)):
            dE = ops.linear(dtab, w[:, col0:col0 + h].t().contiguous(), None, out=dE, out_dtype=F32, residual=dE, exact=True)
            ops.gemm(dtab.t().contiguous(), e_t, dW, D, h, V, c_off=col0, c_row=(0, 0, K), exact=True)
        ops.copy(dsep, dW[:, 2 * h])
        grads = {self.embed_seq.weight: dE, self.proj.weight: dW, self.proj.bias: dbias}
        dtempl = None
        if self.use_template:
            lnm = self.ln_template
            s = _grad_scale([g])
            gt = g if T() == F32 else ops.axpby(g, s, None, 0.0, torch.empty(g.shape, device=dev, dtype=T()))
            dwt, _ = ops.conv_wgrad(gt, tape["tn"], 1)
            wt_t = self.cached("wtempl_t", lambda: self.proj.weight.detach()[:, 2 * h + 1:].t().to(T()).contiguous())
            dtn = ops.linear(gt, wt_t, None, out_dtype=F32, exact=True)
            dtempl, dgamma, dbeta = ops.layernorm_bwd(tape["template"], dtn, _f(lnm.weight), eps=lnm.eps)
            _unscale([dwt, dgamma, dbeta, dtempl if want_template else None], s)
            ops.copy(dwt, dW[:, 2 * h + 1:])
            grads.update({lnm.weight: dgamma, lnm.bias: dbeta})
        return dtempl if want_template else None, grads

    def _backward_from_autograd(self, tape, gs, s, want):
        dtempl, grads = self._backward(tape, _f32_gradient(gs[0]), want_template=bool(want[2]))
        return (None, None, dtempl), grads


# ================================================================================================
# MSA row (tied) attention
# ================================================================================================
class PositionWiseWeightFactor(RecordingModule):
    """rf.py:184-217.  enable_backward(): with grad mode on, forward(msa_emb) records on the direct form (weights()), and
    loss.backward() fills the .grad of to_q and to_k and of msa_emb where it requires grad, through rf_poswise_bwd
    (include/rfmi.h); in train() mode the backward replays the dropout on the softmax weights.  to_k's bias moves every logit of a
    softmax by the same amount: its gradient is the sum of terms that cancel, zero up to their rounding.  d_msa must be a multiple
    of 8 while recording.  The attention layers and the structure track call weights() / weights_head_major() /
    weights_collapsed() without a tape: RoseTTAFold.forward never records here.  (A recording SoftTiedAttentionOverResidues
    hands weights_head_major() / drop() a dict for the dropout record alone and composes _backward itself.)"""

    def __init__(self, d_msa=384, n_heads=12, p_dropout=0.1):
        super().__init__()
        assert d_msa % n_heads == 0, \
            f"[{self.__class__.__name__}]: d_msa ({d_msa}) must be divisible by n_heads ({n_heads})."
        self.n_heads = n_heads
        self.d_head = d_msa // n_heads
        self.scale = self.d_head ** (-0.5)
        self.p_dropout = p_dropout
        self.to_q = nn.Sequential(Linear(d_msa, d_msa), nn.Identity())
        self.to_k = nn.Sequential(Linear(d_msa, d_msa), nn.Identity())

    def drop(self, w, tape=None):
        """rf.py:217: dropout on the softmax weights (training mode; they then no longer sum to one, as in the reference).
        tape: receives the dropout's (p, seed, offset) record as "drop" (None: nothing was dropped)."""
        if tape is not None:
            tape["drop"] = _dropout_rec(w, self.p_dropout) if self.training else None
            return w
        return dropout_(w, self.p_dropout) if self.training else w

    def query_proj(self, xn):
        """to_q on MSA row 0 only: [B*L, d] (T)."""
        B, N, Lr, D = xn.shape
        q0 = torch.empty(B * Lr, D, device=xn.device, dtype=T())
        ops.gemm(xn, self.wt("q", self.to_q[0]), q0, B * Lr, D, D, a_row=(Lr, N * Lr * D, D),
                 bias=_f(self.to_q[0].bias))
        return q0

    def weights(self, xn, w_out=None, tape=None):
        """xn: T [B,N,L,d] -> w fp32 [B,N,H,L].  tape: a dict that receives what _backward needs (the input and the dropout
        record; same kernels, same numbers)."""
        B, N, Lr, D = xn.shape
        _check_backward_call(self, tape, None, D)
        q0 = self.query_proj(xn)
        k = ops.linear(xn, self.wt("k", self.to_k[0]), _f(self.to_k[0].bias))
        w = torch.empty(B, N, self.n_heads, Lr, device=xn.device, dtype=F32) if w_out is None else w_out
        ops.poswise(q0, D, k, D, 0, self.d_head, self.d_head, w, None, 0, 0, 0, B, N, Lr, self.n_heads, self.scale, 1.0)
        if tape is not None:
            tape["xn"] = xn
        return self.drop(w, tape)

    def _backward(self, tape, g):
        """g: contiguous fp32 [B, N, H, L] gradient of the weights (read only).  Returns (fp32 d xn [B,N,L,d], {param: grad}).
        With q0 and k rebuilt from the saved input by the forward's two projections:
            dq0, dk = rf_poswise_bwd(q0, k, g)                          (the dropout record replayed)
            dW_k, db_k = dk^T xn, sum dk;   dW_q, db_q = dq0^T xn_0, sum dq0     rf_conv_wgrad
            d xn = dk W_k;   d xn[:, 0] += dq0 W_q                      rf_gemm"""
        xn = tape["xn"]
        B, N, Lr, D = xn.shape
        H, dh = self.n_heads, self.d_head
        lq, lk = self.to_q[0], self.to_k[0]
        q0 = self.query_proj(xn)
        k = ops.linear(xn, self.wt("k", lk), _f(lk.bias))
        dq0, dk = ops.poswise_bwd(q0, D, k, D, 0, dh, dh, B, N, Lr, H, self.scale, dw=g, dk_dtype=T(), dropout=tape["drop"])
        del q0, k
        dq0_t = ops.cast(dq0.view(B * Lr, D), T())
        x0 = torch.empty(B, Lr, D, device=xn.device, dtype=T())     # xn[:, 0]
        ops.copy(xn[:, 0], x0)
        grads = {}
        grads[lk.weight], grads[lk.bias] = ops.conv_wgrad(dk, xn, 1, bias=True)
        grads[lq.weight], grads[lq.bias] = ops.conv_wgrad(dq0_t, x0.view(B * Lr, D), 1, bias=True)
        dx = ops.linear(dk, self.wt_input_grad("k", lk), None, out_dtype=F32, exact=True)
        dx0 = ops.linear(dq0_t, self.wt_input_grad("q", lq), None, out_dtype=F32, exact=True).view(B, Lr, D)
        for b in range(B):
            ops.axpby(dx[b, 0], 1.0, dx0[b], 1.0, dx[b, 0])
        return dx, grads

    def weights_head_major(self, xn, tape=None):
        """xn: T [B,N,L,d] -> w fp32 [B,H,N,L], without the to_k projection over the N rows: per head
        u[b,l,h,:] = W_k[h*dh:(h+1)*dh, :]^T to_q(x_0)[b,l,h*dh:(h+1)*dh], w = softmax_n(scale * xn . u)   (rf.py:205-217,
        collapsed; to_k's bias is constant over n and drops out of the softmax).  tape: receives the dropout's record (drop()):
        the mask was drawn over THIS layout, [B,H,N,L]."""
        B, N, Lr, D = xn.shape
        H, dh = self.n_heads, self.d_head
        q0 = self.query_proj(xn)
        wkt = self.cached("wkT", lambda: self.to_k[0].weight.detach().t().contiguous().to(T()))
        u = torch.empty(B, Lr, H, D, device=xn.device, dtype=T())
        ops.gemm(q0, wkt, u, B * Lr, D, dh, batch=(H, 1, 1), a_bs=(dh, 0, 0), a_row=(0, 0, D), b_bs=(dh, 0, 0),
                 b_row=(0, 0, D), c_bs=(D, 0, 0), c_row=(0, 0, H * D))
        return self.drop(ops.poswise_collapsed(xn, u, self.scale), tape)

    def weights_collapsed(self, msa, lnm, m, tape=None):
        """1-head weights for the structure track, q side in fp32: w = softmax_n(scale * m[b,n,l,:] . u[b,l,:]) with
        u = to_q(LN(msa[:,0])) W_k  (to_k's bias is constant over n and drops out of the softmax).
        msa fp32 [B,N,L,D]; lnm = the LayerNorm applied to it; m = lnm(msa) in T.
        tape: a dict that receives what _node_input_backward needs (row 0 normalised, q0, u and the dropout record; same
        kernels, same numbers)."""
        assert self.n_heads == 1
        B, N, Lr, D = msa.shape
        row0 = ops.layernorm(msa[:, 0].contiguous(), _f(lnm.weight), _f(lnm.bias), eps=lnm.eps, out_dtype=F32)
        q0 = ops.linear(row0, self.to_q[0].weight.detach().float(), _f(self.to_q[0].bias), out_dtype=F32)
        wkt = self.cached("wkt32", lambda: self.to_k[0].weight.detach().float().t().contiguous())
        u = ops.linear(q0, wkt, None, out_dtype=F32)
        w = torch.empty(B, N, 1, Lr, device=msa.device, dtype=F32)
        ops.poswise(u, D, m, D, 0, 0, D, w, None, 0, 0, 0, B, N, Lr, 1, self.scale, 1.0)
        if tape is not None:
            tape.update(row0=row0, q0=q0, u=u)
        return self.drop(w, tape)

    def _record(self, msa_emb, tape):
        w = self.weights(ops.cast(msa_emb.contiguous(), T()), tape=tape)
        return w.unsqueeze(-1)  # b N h l 1

    def _backward_from_autograd(self, tape, gs, s, want_dx):
        B, N, Lr, _ = tape["xn"].shape
        dx, grads = self._backward(tape, _scaled_copy(gs[0], s).view(B, N, self.n_heads, Lr))
        _unscale([dx], s)
        return dx, grads


# Shortest chain that fills no tile of the fused tied-attention kernels (ops.TIED_TILES) and still takes them, on their tail
# instantiations; below it the general path (rf_gemm + rf_tied_softmax + attention_values) runs.  See DESIGN.md 7g.
TIED_RAGGED_MIN_L = 40


class SoftTiedAttentionOverResidues(RecordingModule):
    """rf.py:220-267.  enable_backward() (switches `poswise_weight` along): with grad mode on, forward(x) records -- on whichever
    route the shape takes -- and loss.backward() fills the .grad of every parameter and of x where it requires grad; with
    return_att both outputs take part in autograd and either gradient may be missing.  The backward (_backward) rebuilds its
    operands from the saved input on the general route and differentiates the unconditioned function: value_conditioning is an
    identity for any constant.  to_k.bias and poswise_weight.to_k.bias get exact zeros: each adds a constant to every logit of
    a softmax row.  d_msa and d_msa / n_heads must be multiples of 8 while recording.  EncoderLayer.run and everything above it
    call attend() without a tape: they never record here.

    attend() runs the route that route(B, N, L) names (ROUTES).  The stages the routes share are written once: maps,
    value_biases, head_major_front, into_residual, and general_operands for the training-mode forward and _backward."""
    ROUTES = ("head_major", "long_rows", "general_fused_logits", "general")

    def __init__(self, d_msa=384, n_heads=12, p_dropout=0.1, return_att=False):
        super().__init__()
        assert d_msa % n_heads == 0, \
            f"[{self.__class__.__name__}]: d_msa ({d_msa}) must be divisible by n_heads ({n_heads})."
        self.n_heads, self.d_head = n_heads, d_msa // n_heads
        self.scale = self.d_head ** (-0.5)
        self.return_att = return_att
        self.p_dropout = p_dropout
        self.poswise_weight = PositionWiseWeightFactor(d_msa, n_heads, p_dropout)
        self.to_q = Linear(d_msa, d_msa)
        self.to_k = Linear(d_msa, d_msa)
        self.to_v = Linear(d_msa, d_msa)
        self.to_out = Linear(d_msa, d_msa)

    def attend(self, xn, x_res, want_att, next_ln=None, drops=(), tape=None):
        """xn: T [B,N,L,D] (already layer-normed); x_res: fp32 [B,N,L,D] += to_out(attention).  Returns
        (symmetrised attention map fp32 [B,L,L,H] when want_att, next_ln(x_res) when fused else None).
        Training mode: the position weights are dropped out inside (rf.py:217); `drops` = the dropouts on the projected output
        before the residual add (this module's own, rf.py:265-267, and the wrapping EncoderLayer's, rf.py:346).
        tape: a dict that receives what _backward needs -- xn, the output dropouts' records ("drops"), the position weights'
        dropout record ("pw") and the layout its mask was drawn over ("w_order": "bhnl" on the head-major and long-row routes,
        "bnhl" on the general one) -- while the route the shape takes runs unchanged: same kernels, same numbers."""
        B, N, Lr, D = xn.shape
        _check_backward_call(self, tape, None, D, self.d_head)
        route = self.route(B, N, Lr)
        if tape is not None:
            tape.update(xn=xn, drops=[], pw={"drop": None}, w_order="bnhl" if route.startswith("general") else "bhnl")
        if route.startswith("general"):
            return self.attend_general(xn, x_res, want_att, next_ln, drops, tape, fused_logits=route == "general_fused_logits")
        return (self.attend_head_major if route == "head_major" else self.attend_long_rows)(xn, x_res, want_att, next_ln, drops, tape)

    def route(self, B, N, Lr):
        """The one of ROUTES that attend() takes at xn [B,N,L,D] ("general_fused_logits": the general route with
        rf_tied_logits_softmax), from the shape, T(), the RT switches and the ops.*_applies predicates: no tensor, no launch.
        tests/golden/tied_routes.json holds its answers over a grid, quirks included: a whole tile counts the position-weight
        tile in LDS even when the weights are folded into q, and has floors on the row count that other chains lack."""
        H, dh, rows, h16, tile = self.n_heads, self.d_head, B * N * Lr, ops.is_h16(T()), Lr in ops.TIED_TILES
        D = H * dh
        # (any MSA depth 1 <= N <= 256: rf_poswise_collapsed pads its last tile of 16 rows inside the kernel; weights applied in
        # the logits kernel are staged four MSA rows at a time, so a depth off a multiple of 4 needs them folded into q)
        if RT.fused_tied and RT.tied_v2 and H <= 16 and 1 <= N <= 256:
            fold = self.folds_weights(rows)
            if tile:
                if (h16 and dh == 32 and (N % 4 == 0 or fold) and rows % 256 == 0 and rows >= 16384
                        and ops.tied_lds_fits(Lr, N)):
                    return "head_major"
            elif Lr >= TIED_RAGGED_MIN_L and ops.tied_fused_applies(Lr, N, T(), dh, w=not fold):
                # a chain that fills no tile: the same route on the tail instantiations of the kernels (rf_tied_attention_ld)
                return "head_major"
            # (the projection is the only kernel on the long-row route with a condition on the row count, B * N * Lr % 64 == 0
            # and >= 16384, and gemm_takes_row_scale states it)
            if (RT.tied_fold_w and 256 < Lr <= 1024 and (Lr in (512, 768, 1024) or RT.tied_long_ragged)
                    and ops.tied_long_applies(Lr, N, T(), dh) and ops.gemm_takes_row_scale(rows, 2 * D, D)):
                return "long_rows"
        return "general_fused_logits" if RT.fused_tied and h16 and dh == 32 and tile else "general"

    # the stages every route shares ---------------------------------------------------------------------------------------------
    def maps(self, B, Lr, dev, want_att):
        """(att T [B,H,L,map_ld(L)]: the kernel that fills it writes zeros in the pad columns; fp32 [B,L,L,H] for the symmetrised
        map when wanted, else None)"""
        return (torch.empty(B, self.n_heads, Lr, map_ld(Lr), device=dev, dtype=T()),
                torch.empty(B, Lr, Lr, self.n_heads, device=dev, dtype=F32) if want_att else None)

    def value_biases(self, xn, lead=(), h16_only=False):
        """(bias of the projection whose output columns are [lead..., v], bias of to_out): value_conditioning's where it is switched
        on, else the plain ones.  h16_only: the general route also runs in float32 and conditions in the 16-bit modes only."""
        if RT.condition and RT.condition_values and (ops.is_h16(T()) or not h16_only):
            return tuple(t_[0] for t_ in self.value_conditioning(xn, self.to_v, self.to_out, lead=lead))
        return (self.bcat("qkv", [*lead, self.to_v]) if lead else _f(self.to_v.bias)), _f(self.to_out.bias)

    def into_residual(self, out, bo, x_res, next_ln, drops, tape):
        """x_res += to_out(out) with the output dropouts (their records onto the tape) -> next_ln(x_res) when fused, else None"""
        return project_into_residual(out, self.wt("o", self.to_out), bo, x_res, next_ln, drops,
                                     recs=tape["drops"] if tape is not None else None)

    def head_major_front(self, xn, key, lins, fold, tape):
        """Both head-major routes: the position weights w fp32 [B,H,N,L] from the collapsed form (no to_k projection over the N
        rows) and one GEMM projecting `lins` (q | k | v or q | k) head-major, [B,N,G,L,32] with G = len(lins) * H: every
        contraction step of the attention kernels is then one contiguous tile.  fold: q * w * d_head^-0.5 (rf.py:252) in that
        GEMM's epilogue, on the fp32 accumulators, so q is rounded once and the logits kernel sees no weights.
        -> (w, the projection, to_out's bias from value_biases when v is projected here, else None)"""
        B, N, Lr, D = xn.shape
        H, dh, G = self.n_heads, self.d_head, len(lins) * self.n_heads
        w = self.poswise_weight.weights_head_major(xn, tape["pw"] if tape is not None else None)
        proj = torch.empty(B, N, G, Lr, dh, device=xn.device, dtype=T())
        if not fold and Lr % 4:
            # the logits kernel stages w by 16-byte pieces: rows padded to a multiple of 4 floats (the pad is read, its values
            # scale query rows past the chain only, which are never stored)
            Lw = (Lr + 3) // 4 * 4
            w_pad = ops.zeros(B, H, N, Lw, device=xn.device, dtype=F32)
            ops.copy(w, w_pad[..., :Lr])
            w = w_pad
        bias, bo = self.value_biases(xn, lead=lins[:-1]) if lins[-1] is self.to_v else (self.bcat(key, lins), None)
        ops.gemm(xn, self.wcat(key, lins), proj, B * N * Lr, len(lins) * D, D, bias=bias, c_row=(Lr, G * Lr * dh, dh),
                 c_col=(dh, Lr * dh), rs=(w, H * N * Lr, N * Lr, dh, D, self.scale) if fold else None)
        return w, proj, bo

    def general_operands(self, xn, drop=None):
        """The general route's operands: one GEMM for q | k | poswise-k [B,N,L,3D], w = softmax_n(q0 . k_pw * scale) and q~ = q w
        d_head^-0.5 (rf.py:252).  drop None: the poswise kernel writes q~ over the q block and w never exists as a tensor;
        returns (qkp, None, None).  Else drop(w) drops w fp32 [B,N,H,L] in place between the softmax and the scaling; returns
        (qkp with q as projected, the dropped weights per (token, head) fp32 [B,N,L,H], q~ T [B,N,L,D])."""
        B, N, Lr, D = xn.shape
        H, dh, dev, W3 = self.n_heads, self.d_head, xn.device, 3 * D
        pw = self.poswise_weight
        lins = [self.to_q, self.to_k, pw.to_k[0]]
        qkp = ops.linear(xn, self.wcat("qkp", lins), self.bcat("qkp", lins))
        q0 = pw.query_proj(xn)
        if drop is None:
            ops.poswise(q0, D, qkp, W3, 2 * D, dh, dh, None, qkp, W3, 0, dh, B, N, Lr, H, pw.scale, self.scale)
            return qkp, None, None
        w = torch.empty(B, N, H, Lr, device=dev, dtype=F32)
        ops.poswise(q0, D, qkp, W3, 2 * D, dh, dh, w, None, 0, 0, 0, B, N, Lr, H, pw.scale, 1.0)
        drop(w)
        wl = ops.copy(w.transpose(2, 3), torch.empty(B, N, Lr, H, device=dev, dtype=F32))
        del w
        qt = ops.copy(qkp[..., :D], torch.empty(B, N, Lr, D, device=dev, dtype=T()))
        ops.scale_rows(qt, ops.axpby(wl, self.scale, None, 0.0, torch.empty_like(wl)), B * N * Lr * H, dh, out=qt)
        return qkp, wl, qt

    def attend_general(self, xn, x_res, want_att, next_ln=None, drops=(), tape=None, fused_logits=False):
        """Any shape and compute dtype: q | k | poswise-k row-major, v key-contiguous, the logits from rf_tied_logits_softmax
        (fused_logits) or rf_gemm + rf_tied_softmax, attention . V on rf_gemm."""
        B, N, Lr, D = xn.shape
        H, dh, W3 = self.n_heads, self.d_head, 3 * D
        pw = self.poswise_weight
        # training mode: the weights exist as a tensor so that the dropout can sit between the softmax and the scaling
        dropping = pw.training and pw.p_dropout and pw.p_dropout > 0
        qkp, _, qt = self.general_operands(xn, (lambda w: pw.drop(w, tape["pw"] if tape is not None else None)) if dropping else None)
        if dropping:
            ops.copy(qt, qkp[..., :D])
        bv, bo = self.value_biases(xn, h16_only=True)
        v_t = self.values_transposed(self.to_v, xn, bv)
        # logits[b,h,i,j] = sum_{n,d} q k   (contraction over N*dh, rf.py:254), softmax over j (rf.py:255)
        att, att_sym = self.maps(B, Lr, xn.device, want_att)
        if fused_logits:
            # one launch: 6-8-stage DMA ring over the N steps, logits in registers, wave-local softmax (csrc/tied.hip)
            ops.tied_logits_softmax(qkp, qkp[..., D:], N * Lr * W3, Lr * W3, W3, att, att_sym, B, H, N, Lr, dh)
        else:
            logits = torch.empty(B, H, Lr, Lr, device=xn.device, dtype=F32)
            ops.gemm(qkp, qkp, logits, Lr, Lr, N * dh, batch=(B, H, 1), b_off=D,
                     a_bs=(N * Lr * W3, dh, 0), a_row=(0, 0, W3), a_ko=Lr * W3,
                     b_bs=(N * Lr * W3, dh, 0), b_row=(0, 0, W3), b_ko=Lr * W3, kc=dh,
                     c_bs=(H * Lr * Lr, Lr * Lr, 0), c_row=(0, 0, Lr))
            ops.tied_softmax(logits, att, att_sym, H)
        return att_sym, self.into_residual(self.attention_values(att, v_t), bo, x_res, next_ln, drops, tape)

    def folds_weights(self, rows):
        """the head-major q|k|v projection of `rows` MSA positions folds w * d_head^-0.5 into q (attend_head_major)"""
        D = self.n_heads * self.d_head
        return RT.tied_fold_w and self.d_head % 16 == 0 and ops.gemm_takes_row_scale(rows, 3 * D, D)

    def attention_values(self, att, v_t):
        """out[b,n,i,(h,d)] = sum_j att[b,h,i,j] v[b,n,h,j,d]   (rf.py:257-258): att T [B,H,L,Lp], v_t T [B,N,D,Lp]
        (values_transposed; Lp = map_ld(L): the contraction runs over Lp, both operands hold zeros in their pad columns)
        -> T [B,N,L,D], one GEMM per (b, head) over all N rows."""
        B, N, D, Lp = v_t.shape
        Lr = att.shape[2]
        H, dh = self.n_heads, self.d_head
        out = torch.empty(B, N, Lr, D, device=v_t.device, dtype=T())
        ops.gemm(att, v_t, out, Lr, N * dh, Lp, batch=(B, H, 1),
                 a_bs=(H * Lr * Lp, Lr * Lp, 0), a_row=(0, 0, Lp),
                 b_bs=(N * D * Lp, dh * Lp, 0), b_row=(dh, D * Lp, Lp),
                 c_bs=(N * Lr * D, dh, 0), c_row=(0, 0, D), c_col=(dh, Lr * D))
        return out

    def attend_head_major(self, xn, x_res, want_att, next_ln=None, drops=(), tape=None):
        """The bench path (csrc/tied.hip), any L <= 256: head_major_front with q | k | v, the position weights folded into q or
        applied inside the logits kernel, attention . V consuming v with transposed LDS reads: no v^T GEMM, no pass over q, no
        fp32 logits."""
        B, N, Lr, D = xn.shape
        H, dh = self.n_heads, self.d_head
        # (folded where the projection runs on the kernel whose epilogue knows the row-group scale; d_msa = 288, N = 864: not)
        fold = self.folds_weights(B * N * Lr)
        w, qkv, bo = self.head_major_front(xn, "qkv", [self.to_q, self.to_k, self.to_v], fold, tape)
        att, att_sym = self.maps(B, Lr, xn.device, want_att)
        out = torch.empty(B, N, Lr, D, device=xn.device, dtype=T())
        ops.tied_attention(qkv[:, :, 0:H], qkv[:, :, H:2 * H], qkv[:, :, 2 * H:], out.view(B, N, Lr, H, dh).permute(0, 1, 3, 2, 4),
                           att, w=None if fold else w, qscale=1.0 if fold else self.scale, att_sym=att_sym)
        return att_sym, self.into_residual(out, bo, x_res, next_ln, drops, tape)

    def attend_long_rows(self, xn, x_res, want_att, next_ln=None, drops=(), tape=None):
        """Any 256 < L <= 1024 (L in {512, 768, 1024}: BASELINE.json configs[3]; every other length runs the tail instantiations
        of the same kernel through ops.tied_logits_long, with the map's row pitch map_ld(L)): head_major_front with q | k and the
        weights folded into q, then the contraction-split logits kernel over 128-query x 256-key tiles (csrc/tied.hip:
        rf_tied_logits, rf_tied_logits_long).  attention . V at these lengths is a plain large GEMM per (b, head) (M = L queries,
        K = L keys, N = n_seq * 32): it goes to rf_gemm with v written key-contiguous by its projection (whole probability
        rows in registers, as in the L <= 256 kernel, would need 128 VGPRs per 16 query rows)."""
        B, N, Lr, D = xn.shape
        H = self.n_heads
        _, qk, _ = self.head_major_front(xn, "qk", [self.to_q, self.to_k], True, tape)
        att, att_sym = self.maps(B, Lr, xn.device, want_att)
        (ops.tied_logits if Lr in (512, 768, 1024) else ops.tied_logits_long)(qk[:, :, 0:H], qk[:, :, H:], att, att_sym)
        bv, bo = self.value_biases(xn)
        out = self.attention_values(att, self.values_transposed(self.to_v, xn, bv))
        return att_sym, self.into_residual(out, bo, x_res, next_ln, drops, tape)

    def _replay_weight_dropout(self, t, tape):
        """t: fp32 [B,N,H,L], the position weights or their gradient (in place): times the forward's keep / (1 - p).  The Philox
        mask follows the element offset, so it is replayed over the layout the forward dropped the weights in (tape["w_order"])."""
        rec = tape["pw"]["drop"]
        if rec is None:
            return t
        if tape["w_order"] == "bnhl":
            return _replay_dropout(t, rec)
        B, N, H, Lr = t.shape
        hm = ops.copy(t.transpose(1, 2), torch.empty(B, H, N, Lr, device=t.device, dtype=F32))
        _replay_dropout(hm, rec)
        ops.copy(hm, t.transpose(1, 2))
        return t

    def _backward(self, tape, g, g_sym=None):
        """g: contiguous fp32 [B,N,L,D], the gradient of what attend() added to x_res (overwritten); g_sym: contiguous fp32
        [B,L,L,H], the gradient of the symmetrised map, or None.  Returns (fp32 d xn [B,N,L,D], {param: grad}).  q | k |
        poswise-k, the (dropped) position weights w, q~ = q w d_head^-0.5, v, v^T and the fp32 logits are rebuilt from the saved
        xn on the general route, whichever route the forward took, with the plain biases.  Then, with s = d_head^-0.5:
            dW_o, db_o = g^T o, sum g;   do = g W_o                                rf_conv_wgrad, rf_gemm
            dp = sum_{n,d} do v                                                     rf_gemm, K = N * d_head in chunks of d_head
            ds = p (dp + sym(g_sym) - sum p (dp + sym(g_sym)))                      rf_tied_softmax_bwd (p, ds also 16-bit)
            dv = p^T do;   dq~ = ds k;   dk = ds^T q~                               rf_gemm over the chain (map_ld, zero pads)
            dq = s w dq~;   dw = s sum_d dq~ q                                      rf_scale_rows_bwd
            d xn_pw, grads = poswise_weight._backward(dw, the mask replayed)        rf_poswise_bwd
            dW_{q,k,v}, db_{q,v} = [dq | dk | dv]^T xn;   db_k = 0 exactly          rf_conv_wgrad
            d xn = [dq | dk | dv] [W_q; W_k; W_v] + d xn_pw                         rf_gemm, exact fp32"""
        xn = tape["xn"]
        B, N, Lr, D = xn.shape
        H, dh = self.n_heads, self.d_head
        dev = xn.device
        pw = self.poswise_weight
        W3, Lp, R = 3 * D, map_ld(Lr), B * N * Lr
        h16 = ops.is_h16(T())
        for rec in tape["drops"]:
            _replay_dropout(g, rec)
        g_t = ops.cast(g.view(R, D), T())

        # ---- the forward's operands, general route
        qkp, wl, qt = self.general_operands(xn, lambda w: self._replay_weight_dropout(w, tape))
        logits = torch.empty(B, H, Lr, Lr, device=dev, dtype=F32)
        tied_k = dict(batch=(B, H, 1), kc=dh, c_bs=(H * Lr * Lr, Lr * Lr, 0), c_row=(0, 0, Lr))   # a contraction over N * dh
        rows_d = lambda ld_: dict(bs=(N * Lr * ld_, dh, 0), row=(0, 0, ld_), ko=Lr * ld_)   # noqa: E731  (head h of [B,N,L,ld_])
        a_d, b_w3 = ({f"a_{k_}": v_ for k_, v_ in rows_d(D).items()}, {f"b_{k_}": v_ for k_, v_ in rows_d(W3).items()})
        ops.gemm(qt, qkp, logits, Lr, Lr, N * dh, b_off=D, **a_d, **b_w3, **tied_k)
        v = ops.linear(xn, self.wt("v", self.to_v), _f(self.to_v.bias))          # the values row-major [B,N,L,D]

        def key_contiguous(src, off=0):
            """columns off.. of [B,N,L,(h,d)] rows -> [B,N,D,Lp]: the B operand of a contraction over the chain (zero pads)"""
            dst = (torch.empty if Lp == Lr else ops.zeros)(B, N, D, Lp, device=dev, dtype=T())
            ops.copy(src[..., off:off + D].transpose(2, 3), dst[..., :Lr])
            return dst

        def map_transposed(m):
            """[B,H,L,Lp] -> the same with rows and columns swapped (zero pads)"""
            dst = (torch.empty if Lp == Lr else ops.zeros)(B, H, Lr, Lp, device=dev, dtype=m.dtype)
            ops.copy(m[..., :Lr].transpose(2, 3), dst[..., :Lr])
            return dst

        def over_chain(m, bt, out, ld_, off):
            """out[b,n,i,off + (h,d)] = sum_j m[b,h,i,j] bt[b,n,(h,d),j]: attention_values into rows of ld_"""
            return ops.gemm(m, bt, out, Lr, N * dh, Lp, batch=(B, H, 1), c_off=off, exact=True,
                            a_bs=(H * Lr * Lp, Lr * Lp, 0), a_row=(0, 0, Lp),
                            b_bs=(N * D * Lp, dh * Lp, 0), b_row=(dh, D * Lp, Lp),
                            c_bs=(N * Lr * ld_, dh, 0), c_row=(0, 0, ld_), c_col=(dh, Lr * ld_))

        # ---- output projection, d p, the softmax and the symmetrised map
        do = ops.linear(g_t, self.wt_input_grad("o", self.to_out), None, exact=True).view(B, N, Lr, D)
        dp = torch.empty(B, H, Lr, Lr, device=dev, dtype=F32)
        ops.gemm(do, v, dp, Lr, Lr, N * dh, exact=True, **a_d, **{f"b_{k_}": v_ for k_, v_ in rows_d(D).items()}, **tied_k)
        ds, p, ds_t = ops.tied_softmax_bwd(logits, dp, g_sym, h16_copies=h16)
        if not h16:
            p, ds_t = torch.empty(B, H, Lr, Lr, device=dev, dtype=F32), ds
            ops.tied_softmax(logits, p)
        del logits, dp
        grads = {}
        o = over_chain(p, key_contiguous(v), torch.empty(B, N, Lr, D, device=dev, dtype=T()), D, 0)
        grads[self.to_out.weight], grads[self.to_out.bias] = ops.conv_wgrad(g_t, o.view(R, D), 1, bias=True)
        del o, v, g_t
        # ---- dq~, then dq | dk | dv in the layout of a q | k | v projection
        dqt = over_chain(ds_t, key_contiguous(qkp, D), torch.empty(B, N, Lr, D, device=dev, dtype=T()), D, 0)
        dqkv = torch.empty(B, N, Lr, W3, device=dev, dtype=T())
        over_chain(map_transposed(ds_t), key_contiguous(qt), dqkv, W3, D)
        over_chain(map_transposed(p), key_contiguous(do), dqkv, W3, 2 * D)
        del ds, ds_t, p, do, qt
        _, dwl = ops.scale_rows_bwd(qkp, W3, dh, dqt, D, dh, wl.view(-1), self.scale, R, H, dh, dx=dqkv, dx_ld=W3, dx_hs=dh)
        del dqt, qkp, wl
        # ---- the position weights
        dw = torch.empty(B, N, H, Lr, device=dev, dtype=F32)
        ops.copy(dwl.view(B, N, Lr, H), dw.transpose(2, 3))
        self._replay_weight_dropout(dw, tape)
        dxn, gpw = pw._backward({"xn": xn, "drop": None}, dw)
        gpw[pw.to_k[0].bias] = ops.zeros(D, device=dev, dtype=F32)
        grads.update(gpw)
        # ---- the three projections
        dwqkv, dbqkv = ops.conv_wgrad(dqkv.view(R, W3), xn.view(R, D), 1, bias=True)
        for i, lin in enumerate((self.to_q, self.to_k, self.to_v)):
            grads[lin.weight], grads[lin.bias] = dwqkv[i * D:(i + 1) * D], dbqkv[i * D:(i + 1) * D]
        grads[self.to_k.bias] = ops.zeros(D, device=dev, dtype=F32)
        wqkv_t = self.cached(("wqkv_input_grad",), lambda: torch.cat([lin.weight.detach() for lin in (self.to_q, self.to_k, self.to_v)],
                                                                     0).t().to(T()).contiguous())
        ops.linear(dqkv.view(R, W3), wqkv_t, None, out=dxn.view(R, D), residual=dxn.view(R, D), exact=True)
        return dxn, grads

    def _backward_children(self):
        return (self.poswise_weight,)

    def _record(self, x, tape):
        xn = ops.cast(x.contiguous(), T())
        out = ops.zeros(*x.shape, device=x.device, dtype=F32)
        att, _ = self.attend(xn, out, self.return_att, drops=(self.p_dropout,) if self.training else (), tape=tape)
        return (out, att) if self.return_att else out

    def _backward_from_autograd(self, tape, gs, s, want_dx):
        g_sym = _scaled_copy(gs[1], s) if len(gs) > 1 and gs[1] is not None else None
        dx, grads = self._backward(tape, _scaled_copy(gs[0], s), g_sym)
        _unscale([dx], s)
        return dx, grads


# ================================================================================================
# Performer (FAVOR+) self attention -- restated third-party module (parity unpinned)
# ================================================================================================
class _FastAttention(nn.Module):
    def __init__(self, dim_heads, nb_features):
        super().__init__()
        self.register_buffer("projection_matrix", gaussian_orthogonal_random_matrix(nb_features, dim_heads))


def gaussian_orthogonal_random_matrix(nb_rows, nb_cols, generator=None):
    """performer-pytorch's projection construction (scaling=0); see oracle for the citation."""
    blocks = []
    for _ in range(nb_rows // nb_cols):
        q, _ = torch.linalg.qr(torch.randn(nb_cols, nb_cols, generator=generator), mode="reduced")
        blocks.append(q.t())
    rem = nb_rows - (nb_rows // nb_cols) * nb_cols
    if rem > 0:
        q, _ = torch.linalg.qr(torch.randn(nb_cols, nb_cols, generator=generator), mode="reduced")
        blocks.append(q.t()[:rem])
    mat = torch.cat(blocks)
    mult = torch.randn(nb_rows, nb_cols, generator=generator).norm(dim=1)
    return torch.diag(mult) @ mat


class PerformerSelfAttention(RecordingModule):
    """performer_pytorch.SelfAttention as the reference instantiates it (rf.py:313-318, 505-518):
    dim_head=64, nb_features=266, no qkv bias, output bias; softmax-kernel or generalized ReLU features."""

    def __init__(self, dim, heads=8, dim_head=64, dropout=0.0, generalized_attention=False, **kw):
        super().__init__()
        inner = dim_head * heads
        self.heads, self.dim_head, self.inner = heads, dim_head, inner
        self.p_dropout = dropout   # (performer_pytorch.SelfAttention: nn.Dropout on the projected output)
        self.condition_v = False   # value conditioning of the 16-bit modes (RFModule.value_conditioning): the MSA track switches it on
        self.generalized = generalized_attention
        self.fast_attention = _FastAttention(dim_head, int(dim_head * math.log(dim_head)))
        self.to_q = Linear(dim, inner, bias=False)
        self.to_k = Linear(dim, inner, bias=False)
        self.to_v = Linear(dim, inner, bias=False)
        self.to_out = Linear(inner, dim)

    def proj_scaled(self, log2e=False):
        def make():
            p = self.fast_attention.projection_matrix.detach().float() * self.dim_head ** -0.25
            if log2e:  # the fused softmax-kernel variant exponentiates with exp2
                p = p * 1.4426950408889634
            pp = p.new_zeros(M_PAD, self.dim_head)
            pp[: p.shape[0]] = p
            return pp.to(T()).contiguous()
        return self.cached(("proj", log2e), make)

    def attend(self, xn, x_res, axis, next_ln=None, seq_group=None, drops=(), tape=None):
        """xn: T [B,L1,L2,D] layer-normed input; sequences run along `axis` (1 or 2); x_res (fp32, same shape)
        += to_out(linear attention).  All intermediates are addressed by strides: no transposes.
        Returns next_ln(x_res) when the fused residual+LayerNorm epilogue applies, else None.
        seq_group: a torch.distributed group over which the SEQUENCE axis is sharded (every rank holds a slice of every
        sequence: pair-track row blocks).  Linear attention communicates contexts, not maps: the local
        k'^T [v | 1] sums are all-reduced (fp32) before the queries are applied (rf.py:505-518 semantics unchanged).
        tape: a dict that receives what _backward needs (xn, the axis, the output dropout's records); the kernels are the same."""
        B, D = xn.shape[0], xn.shape[-1]
        _check_backward_call(self, tape, seq_group, D)
        if tape is not None:
            if not self.generalized:
                raise NotImplementedError("PerformerSelfAttention: the backward pass covers the generalized (ReLU) feature map only")
            tape.update(xn=xn, axis=axis, drops=[])
        recs = tape["drops"] if tape is not None else None
        H, dh, inner = self.heads, self.dim_head, self.inner
        geo = self._geometry(xn.shape, axis, seq_group)
        m = self.fast_attention.projection_matrix.shape[0]
        gen = self.generalized
        if seq_group is not None and not gen:
            raise NotImplementedError("sequence-sharded attention is built for the generalized (ReLU) feature map of the pair "
                                      "track only: the softmax feature map needs the global key maximum first")
        cond = RT.condition and RT.condition_values and self.condition_v and ops.is_h16(T()) and seq_group is None
        bqkv, bv, bo = None, None, _f(self.to_out.bias)
        if cond:
            bqkv, bo = (t_[0] for t_ in self.value_conditioning(xn, self.to_v, self.to_out, lead=(self.to_q, self.to_k)))
            bv = bqkv[2 * inner:]
        if seq_group is None and RT.fused_favor and ops.favor_fused_applies(geo.Ls, not gen, dh, m, T()):
            # fused path: one projection GEMM (q|k|v) + one persistent kernel; q', k', ctx never leave the chip (any sequence
            # length: the kernel pads its last tile itself, rows past Ls are neither read nor written)
            Ls, Lo, ss, so, RB = geo.Ls, geo.Lo, geo.ss, geo.so, geo.RB
            W3 = 3 * inner
            o = torch.empty(geo.R, inner, device=xn.device, dtype=T())
            pcf = self.proj_scaled(log2e=not gen)
            eps = 1e-3 if gen else 1e-4
            qkv = ops.linear(xn, self.wcat("qkv", [self.to_q, self.to_k, self.to_v]), bqkv)
            ops.favor_attention(qkv, pcf, o, (RB * W3, so * W3, ss * W3, dh), (RB * inner, so * inner, ss * inner),
                                0, inner, 2 * inner, B, Lo, H, Ls, dh, m, not gen, eps)
            return project_into_residual(o, self.wt("o", self.to_out), bo, x_res, next_ln, drops, recs=recs)
        o = self._linear_attention(xn, geo, bv, seq_group)[-1]
        return project_into_residual(o, self.wt("o", self.to_out), bo, x_res, next_ln, drops, recs=recs)

    def _geometry(self, shape, axis, seq_group=None):
        """How the sequences of xn [B, L1, L2, D] along `axis` are addressed: their length Ls and number per sample Lo, the row
        strides ss / so of the sequence / outer index, rows per sample RB and in all R, sequences times heads S, the q|k row
        width W2 -- and the scale the context is stored with."""
        B, L1, L2, _ = shape
        Ls, Lo = (L1, L2) if axis == 1 else (L2, L1)
        ss, so = (L2, 1) if axis == 1 else (1, L2)
        # fp16 operands (range 65504): the context is a sum over the whole sequence, so it is stored scaled by 2^-ceil(log2 Ls_total)
        # (on the fp32 accumulators, before the rounding) exactly as csrc/favor.hip does in the fused kernel; numerator and
        # denominator of the final ratio carry the same power of two, the result is unchanged
        ctx_scale = 1.0
        if T() == torch.float16:
            from . import shard
            ctx_scale = 2.0 ** -math.ceil(math.log2(max(Ls * (shard.group_size(seq_group) if seq_group is not None else 1), 1)))
        return _SeqGeometry(B, Ls, Lo, ss, so, L1 * L2, B * L1 * L2, B * Lo * self.heads, 2 * self.inner, ctx_scale)

    def _features(self, geo, qk, off, act, dtype):
        """[B, Lo, H, Ls, M_PAD] = act(x P^T), x = the q (off 0) or k (off inner) block of qk: phi with ACT_RELU_EPS, the
        pre-activation z with ACT_NONE (the softmax features' input; in fp32, what the backward masks with)."""
        B, Ls, Lo, ss, so, RB, _, _, W2, _ = geo
        H, dh = self.heads, self.dim_head
        out = torch.empty(B, Lo, H, Ls, M_PAD, device=qk.device, dtype=dtype)
        ops.gemm(qk, self.proj_scaled(), out, Ls * H, M_PAD, dh, batch=(B, Lo, 1), a_off=off,
                 a_bs=(RB * W2, so * W2, 0), a_row=(H, ss * W2, dh),
                 c_bs=(Lo * H * Ls * M_PAD, H * Ls * M_PAD, 0), c_row=(H, M_PAD, Ls * M_PAD),
                 act=act, act_nvalid=self.fast_attention.projection_matrix.shape[0], act_eps=1e-3)
        return out

    def _features_t(self, geo, qk, off, act):
        """The same features transposed, [B, Lo, H, M_PAD, Ls] (sequence index contiguous), in T."""
        B, Ls, Lo, ss, so, RB, _, _, W2, _ = geo
        H, dh = self.heads, self.dim_head
        out = torch.empty(B, Lo, H, M_PAD, Ls, device=qk.device, dtype=T())
        ops.gemm(self.proj_scaled(), qk, out, M_PAD, Ls, dh, batch=(B, Lo, H), b_off=off,
                 b_bs=(RB * W2, so * W2, dh), b_row=(0, 0, ss * W2),
                 c_bs=(Lo * H * M_PAD * Ls, H * M_PAD * Ls, M_PAD * Ls), c_row=(0, 0, Ls),
                 act=act, act_nvalid=-self.fast_attention.projection_matrix.shape[0], act_eps=1e-3)
        return out

    def _linear_attention(self, xn, geo, bv=None, seq_group=None):
        """The unfused chain from xn (bv: the value bias of the conditioned form): returns
        (qk [R, 2 inner], q' [B,Lo,H,Ls,M_PAD], k'^T [B,Lo,H,M_PAD,Ls], [v | 1 | 0]^T [B,Lo,H,80,Ls], context^T [S,80,M_PAD],
        numerator | denominator fp32 [R * H, 80], o [R, inner])."""
        B, Ls, Lo, ss, so, RB, R, S, W2, ctx_scale = geo
        H, dh, inner = self.heads, self.dim_head, self.inner
        dev = xn.device
        D = xn.shape[-1]
        act = L.ACT_RELU_EPS if self.generalized else L.ACT_NONE
        qk = ops.linear(xn, self.wcat("qk", [self.to_q, self.to_k]), None)
        dq = self._features(geo, qk, 0, act, T())
        kt = self._features_t(geo, qk, inner, act)
        if not self.generalized:
            m = self.fast_attention.projection_matrix.shape[0]
            xs = (RB * W2, so * W2, dh, ss * W2)
            ops.favor_softmax_features(dq, qk, 0, xs, Lo, H, S, Ls, m, M_PAD, dh, 1, 0)
            ops.favor_softmax_features(kt, qk, inner, xs, Lo, H, S, Ls, m, M_PAD, dh, 0, 1)
        # v^T [B,Lo,H,80,Ls] with a ones row at index 64 (-> k' column sums ride along in the context GEMM)
        vt = ops.zeros(B, Lo, H, VT_ROWS, Ls, device=dev, dtype=T())
        ones_row = ops.fill(torch.empty(B, Lo, H, Ls, device=dev, dtype=T()), 1.0)
        ops.copy(ones_row, vt[:, :, :, dh])
        ops.gemm(self.wt("v", self.to_v), xn, vt, inner, Ls, D, batch=(B, Lo, 1),
                 b_bs=(RB * D, so * D, 0), b_row=(0, 0, ss * D),
                 c_bs=(Lo * H * VT_ROWS * Ls, H * VT_ROWS * Ls, 0), c_row=(dh, VT_ROWS * Ls, Ls),
                 bias=bv, bias_mode=L.BIAS_ROW)
        # context^T [S,80,M_PAD] = v^T k'
        ctx = torch.empty(S, VT_ROWS, M_PAD, device=dev, dtype=T() if seq_group is None else F32)
        ops.gemm(vt, kt, ctx, VT_ROWS, M_PAD, Ls, batch=(S, 1, 1), a_bs=(VT_ROWS * Ls, 0, 0),
                 b_bs=(M_PAD * Ls, 0, 0), c_bs=(VT_ROWS * M_PAD, 0, 0), alpha=ctx_scale if seq_group is None else 1.0)
        if seq_group is not None:
            # the one exchange of a sequence-sharded layer: [B * Lo * H, 80, 288] fp32 partial contexts (+ k' sums in row 64).
            # The partial sums travel unscaled (the ranks' slices may differ in length); every rank scales its own copy of the
            # full context when it rounds it to the 16-bit type (any power of two cancels in that rank's ratio)
            from . import shard
            shard.all_reduce_sum(ctx, seq_group)
            ctx = ops.axpby(ctx, ctx_scale, None, 0.0, torch.empty(ctx.shape, device=dev, dtype=T()))
        # numerator | denominator: num[b,p1,p2,h,0:64 | 64]
        num = torch.empty(R * H, VT_ROWS, device=dev, dtype=F32)
        ops.gemm(dq, ctx, num, Ls, VT_ROWS, M_PAD, batch=(B, Lo, H),
                 a_bs=(Lo * H * Ls * M_PAD, H * Ls * M_PAD, Ls * M_PAD), a_row=(0, 0, M_PAD),
                 b_bs=(Lo * H * VT_ROWS * M_PAD, H * VT_ROWS * M_PAD, VT_ROWS * M_PAD),
                 c_bs=(RB * H * VT_ROWS, so * H * VT_ROWS, VT_ROWS), c_row=(0, 0, ss * H * VT_ROWS))
        o = torch.empty(R, inner, device=dev, dtype=T())
        ops.linattn_normalize(num, VT_ROWS, o, dh, R * H, dh)
        return qk, dq, kt, vt, ctx, num, o

    def _backward(self, tape, g):
        """g: fp32 [B, L1, L2, D] gradient of what attend() added to x_res (overwritten).  q|k|v, the features, the context and
        the numerator are rebuilt from the saved xn on the unfused chain (whichever forward path ran).  Per sequence, with
        phi = relu(z) + eps, C = phi_k^T [v | 1], N = phi_q C, out = N[:, :64] / N[:, 64]:
            dN = normalize_bwd(N, d out);  dphi_q = dN C^T;  dC = phi_q^T dN;  dphi_k = [v | 1] dC^T;  dv = phi_k dC[:, :64]
            dq = (dphi_q * 1[z_q > 0]) P,  dk = (dphi_k * 1[z_k > 0]) P
        The fp16 mode's context scale s = 2^-ceil(log2 Ls) is carried as in the forward: N and C hold s N, s C, so dN comes out
        as dN / s and dC = s phi_q^T (dN / s).  Returns (fp32 gradient of xn, {param: grad})."""
        xn, axis = tape["xn"], tape["axis"]
        D = xn.shape[-1]
        H, dh, inner = self.heads, self.dim_head, self.inner
        dev = xn.device
        geo = self._geometry(xn.shape, axis)
        B, Ls, Lo, ss, so, RB, R, S, W2, cs = geo
        W3 = 3 * inner
        V = VT_ROWS
        m = self.fast_attention.projection_matrix.shape[0]
        pct = self.cached(("proj_t",), lambda: self.proj_scaled().t().contiguous())   # P^T [dh, M_PAD]
        for rec in tape["drops"]:
            _replay_dropout(g, rec)
        g_t = ops.cast(g.reshape(R, D), T())
        x2 = xn.reshape(R, D)

        # ---- the forward's unfused chain, then the extra layouts the products below contract over
        qk, phq, kt, vt, _, num, o = self._linear_attention(xn, geo)
        zq, zk = self._features(geo, qk, 0, L.ACT_NONE, F32), self._features(geo, qk, inner, L.ACT_NONE, F32)
        phk = self._features(geo, qk, inner, L.ACT_RELU_EPS, T())
        phq_t = self._features_t(geo, qk, 0, L.ACT_RELU_EPS)
        v1 = torch.empty(R * H, V, device=dev, dtype=T())   # [v | 1 | 0] rows in the numerator's row layout
        self._seq_transpose(vt, v1, geo, to_rows=True)
        per_seq = lambda r, c: dict(batch=(S, 1, 1), a_bs=(r, 0, 0), b_bs=(c, 0, 0))   # noqa: E731
        cj = torch.empty(S, M_PAD, V, device=dev, dtype=T())    # C (feature-major; the chain's context is C^T, e-major)
        ops.gemm(kt, vt, cj, M_PAD, V, Ls, c_bs=(M_PAD * V, 0, 0), alpha=cs, **per_seq(M_PAD * Ls, V * Ls))
        num_rows = dict(batch=(B, Lo, H), a_bs=(RB * H * V, so * H * V, V), a_row=(0, 0, ss * H * V))

        # ---- output projection
        dwo, dbo = ops.conv_wgrad(g_t, o, 1, bias=True)
        do = ops.linear(g_t, self.wt_input_grad("o", self.to_out), None, out_dtype=F32, exact=True)   # [R, inner]
        # ---- linear attention
        dn = torch.empty(R * H, V, device=dev, dtype=T())
        ops.linattn_normalize_bwd(num, V, do, dh, dn, V, R * H, dh)
        dn_t = torch.empty(B, Lo, H, V, Ls, device=dev, dtype=T())
        self._seq_transpose(dn_t, dn, geo, to_rows=False)
        dc = torch.empty(S, M_PAD, V, device=dev, dtype=T())     # dC (feature-major)
        ops.gemm(phq_t, dn_t, dc, M_PAD, V, Ls, c_bs=(M_PAD * V, 0, 0), alpha=cs, **per_seq(M_PAD * Ls, V * Ls))
        dc_t = torch.empty(S, V, M_PAD, device=dev, dtype=T())   # dC^T (e-major)
        ops.gemm(dn_t, phq_t, dc_t, V, M_PAD, Ls, c_bs=(V * M_PAD, 0, 0), alpha=cs, **per_seq(V * Ls, M_PAD * Ls))
        feat_c = dict(c_bs=(Lo * H * Ls * M_PAD, H * Ls * M_PAD, Ls * M_PAD))
        dphq = torch.empty(B, Lo, H, Ls, M_PAD, device=dev, dtype=F32)
        ops.gemm(dn, cj, dphq, Ls, M_PAD, V, b_bs=(Lo * H * M_PAD * V, H * M_PAD * V, M_PAD * V), **num_rows, **feat_c)
        dphk = torch.empty(B, Lo, H, Ls, M_PAD, device=dev, dtype=F32)
        ops.gemm(v1, dc, dphk, Ls, M_PAD, V, b_bs=(Lo * H * M_PAD * V, H * M_PAD * V, M_PAD * V), **num_rows, **feat_c)
        dzq = ops.relu_feature_bwd(dphq, zq, m, T())
        dzk = ops.relu_feature_bwd(dphk, zk, m, T())
        del dphq, dphk, zq, zk
        # ---- dq | dk | dv straight into the q|k|v projection's layout [R, 3 inner]
        dqkv = torch.empty(R, W3, device=dev, dtype=T())
        qkv_c = dict(batch=(B, Lo, H), c_bs=(RB * W3, so * W3, dh), c_row=(0, 0, ss * W3))
        feat_a = dict(a_bs=(Lo * H * Ls * M_PAD, H * Ls * M_PAD, Ls * M_PAD))
        ops.gemm(dzq, pct, dqkv, Ls, dh, M_PAD, **feat_a, **qkv_c)
        ops.gemm(dzk, pct, dqkv, Ls, dh, M_PAD, c_off=inner, **feat_a, **qkv_c)
        ops.gemm(phk, dc_t, dqkv, Ls, dh, M_PAD, c_off=2 * inner, b_bs=(Lo * H * V * M_PAD, H * V * M_PAD, V * M_PAD),
                 **feat_a, **qkv_c)
        dw, _ = ops.conv_wgrad(dqkv, x2, 1)   # [3 inner, D]: to_q | to_k | to_v
        wqkv_t = self.cached(("wqkv_input_grad",), lambda: torch.cat([self.to_q.weight.detach(), self.to_k.weight.detach(),
                                                                      self.to_v.weight.detach()], 0).t().to(T()).contiguous())
        dxn = ops.linear(dqkv, wqkv_t, None, out_dtype=F32, exact=True)
        return dxn.view(xn.shape), {self.to_q.weight: dw[:inner], self.to_k.weight: dw[inner:W2], self.to_v.weight: dw[W2:],
                                    self.to_out.weight: dwo, self.to_out.bias: dbo}

    def _seq_transpose(self, seq_major, rows, geo, to_rows):
        """[B, Lo, H, 80, Ls] (sequence index innermost) <-> [B, L1, L2, H, 80] (the numerator's rows), one copy per sample."""
        B, Ls, Lo, ss = geo[:4]
        H, V = self.heads, VT_ROWS
        # both as (b, o, n, h, e): the rows hold (n, o) in that order when the sequences run along axis 1
        r = rows.view(B, Lo, Ls, H, V) if ss == 1 else rows.view(B, Ls, Lo, H, V).transpose(1, 2)
        t = seq_major.permute(0, 1, 4, 2, 3)
        for b in range(B):
            if to_rows:
                ops.copy(t[b], r[b])
            else:
                ops.copy(r[b], t[b])

    def enable_backward(self, mode=True):
        """Opt in to autograd (generalized ReLU feature map only: the softmax-kernel Performer of the MSA track raises
        NotImplementedError): with grad mode on, forward() records and loss.backward() fills the .grad of to_q / to_k / to_v,
        to_out (and of the input, if it requires grad); projection_matrix is a buffer.  Stored on this module; returns self."""
        if mode and not self.generalized:
            raise NotImplementedError("PerformerSelfAttention: the backward pass covers the generalized (ReLU) feature map only")
        return super().enable_backward(mode)

    def _record(self, x, tape):
        """x [S, n, dim] -> [S, n, dim] (library call surface)."""
        S_, n, D = x.shape
        xn = ops.cast(x.contiguous(), T()).view(1, S_, n, D)
        out = ops.zeros(1, S_, n, D, device=x.device, dtype=F32)
        self.attend(xn, out, axis=2, drops=(self.p_dropout,) if self.training else (), tape=tape)
        return out.view(S_, n, D)

    def _backward_from_autograd(self, tape, gs, s, want_dx):
        dx, grads = self._backward(tape, _scaled_copy(gs[0], s).view(tape["xn"].shape))
        _unscale([dx], s)
        return dx.view(gs[0].shape), grads


# ================================================================================================
# encoder layers / MSA self attention update
# ================================================================================================
class EncoderLayer(RFModule):
    """rf.py:284-354."""

    def __init__(self, d_msa=384, d_ff=384 * 4, n_heads=12, p_dropout=0.1, tied=False, performer=False,
                 performer_kws={}, return_att=False):
        super().__init__()
        self.tied, self.return_att = tied, return_att
        if tied:
            self.attn = SoftTiedAttentionOverResidues(d_msa=d_msa, n_heads=n_heads, p_dropout=p_dropout,
                                                      return_att=return_att)
        elif performer:
            if return_att:
                raise NotImplementedError("PerformerSelfAttention does not support return_att.")
            self.attn = PerformerSelfAttention(dim=d_msa, heads=n_heads, dropout=p_dropout, **performer_kws)
            self.attn.condition_v = True
        else:
            raise NotImplementedError
        self.ln = LayerNorm(d_msa)
        self.p_dropout = p_dropout   # rf.py:324,346: x = orig + dropout(attn(ln(x)))
        self.ff = Residual(nn.Sequential(LayerNorm(d_msa), FeedForward(d_msa, d_ff, p_dropout=p_dropout),
                                         nn.Dropout(p_dropout)))

    def run(self, x, seq_axis=2, want_att=False, xn=None, next_ln=None):
        """x: fp32 residual stream [B,n1,n2,D], updated in place.  tied: rows = n1 (MSA depth), attention over n2.
        performer: attention along `seq_axis`.  xn: self.ln(x) if the previous GEMM already produced it;
        next_ln: the LayerNorm that will consume x next.  Returns (att, next_ln(x) or None)."""
        if xn is None:
            xn = ln(self.ln, x)
        att = None
        # training mode: the attention module's own output dropout, then this layer's (rf.py:265-267 / performer, 346); the
        # feed-forward's output dropout (rf.py:330) rides into apply_residual
        ad = (self.attn.p_dropout, self.p_dropout) if self.training else ()
        fd = (_p(self.ff.fn[2]),) if self.training else ()
        if self.tied:
            att, xf = self.attn.attend(xn, x, want_att, next_ln=self.ff.fn[0], drops=ad)
        else:
            xf = self.attn.attend(xn, x, seq_axis, next_ln=self.ff.fn[0], drops=ad)
        if xf is None:
            xf = ln(self.ff.fn[0], x)
        return att, self.ff.fn[1].apply_residual(xf, x, next_ln, drops=fd)

    def forward(self, x):
        x = fresh_f32(x)
        if self.tied:
            att, _ = self.run(x, want_att=self.return_att)
            return (x, att) if self.return_att else x
        # reference flattens (b n) l d: attention along dim 2 of [b, n, l, d]
        self.run(x, seq_axis=2)
        return x


class MsaUpdateUsingSelfAttention(RFModule):
    """rf.py:357-409."""

    def __init__(self, d_msa=384, d_ff=384 * 4, n_heads=12, p_dropout=0.1, n_encoder_layers=4, performer_kws={}):
        super().__init__()
        self.residue_wise_encoder_layers = nn.ModuleList([
            EncoderLayer(d_msa=d_msa, d_ff=d_ff, n_heads=n_heads, p_dropout=p_dropout, tied=True, performer=False,
                         return_att=True) for _ in range(n_encoder_layers)])
        self.sequence_wise_encoder_layers = nn.ModuleList([
            EncoderLayer(d_msa=d_msa, d_ff=d_ff, n_heads=n_heads, p_dropout=p_dropout, tied=False, performer=True,
                         performer_kws=performer_kws) for _ in range(n_encoder_layers)])

    def run(self, x):
        att = None
        layers = list(self.residue_wise_encoder_layers) + list(self.sequence_wise_encoder_layers)
        n = len(self.residue_wise_encoder_layers)
        xn = None
        for i, layer in enumerate(layers):
            nxt = layers[i + 1].ln if i + 1 < len(layers) else None  # the next layer's pre-norm rides in this FF2's epilogue
            if i < n:
                a, xn = layer.run(x, want_att=(i == n - 1), xn=xn, next_ln=nxt)  # only the last map is consumed (rf.py:400-401)
                att = a if a is not None else att
            else:
                # the reference transposes to b l n d: sequences run over the MSA depth
                _, xn = layer.run(x, seq_axis=1, xn=xn, next_ln=nxt)
        return att

    def forward(self, x):
        x = fresh_f32(x)
        return x, self.run(x)


# ================================================================================================
# pair update with MSA (outer product + 2-conv ResNet)
# ================================================================================================
class OuterProductMean(RecordingModule):
    """rf.py:412-427.  enable_backward(): with grad mode on, forward(x, y=None) records, and loss.backward() fills the .grad of
    the LayerNorm and the Linear of to_out and of x and y where they require grad (forward(x): x receives the sum of both
    operands' gradients).  The backward (_backward) rebuilds everything from the 16-bit transposed operands whichever forward
    path ran, in slabs of pair rows (RT.outer_bwd_slab_bytes).  run_rows (a block of rows) is refused while recording, and
    P^2 and out_features must be multiples of 8.  run_into is called by PairUpdateWithMsa.run only, which does not go through
    forward(): it never records, and enable_backward() here changes nothing for the enclosing module."""
    _rf_n_inputs = 2

    def __init__(self, in_features, out_features):
        super().__init__()
        self.to_out = nn.Sequential(LayerNorm(in_features ** 2), Linear(in_features ** 2, out_features))

    def fused_ok(self, P, N, Lr):
        """the fused kernel (csrc/outer.hip) serves this call: 16-bit modes, P = 32, 288 outputs, any chain length Lr >= 1 and
        any MSA depth N <= 128 (run at ops.outer_depth(N) = 64 or 128, zero-padded)"""
        return (RT.fused_outer and ops.is_h16(T()) and P == 32 and 1 <= N <= 128 and Lr >= 1
                and self.to_out[1].weight.shape[0] == 288)

    def depth_multiple(self, P, N, Lr):
        """what ops.outer_operands pads the MSA depth to for the route run() takes: the fused kernel's depth, or 8"""
        return ops.outer_depth(N) if self.fused_ok(P, N, Lr) else 8

    def _fused_operands(self, x_t, y_t):
        """operands at the fused kernel's depth (callers that built them through depth_multiple hand them over as they are)"""
        Nk = ops.outer_depth(x_t.shape[-1])
        return ops.outer_pad_depth(x_t, Nk), ops.outer_pad_depth(y_t, Nk)

    def _fold(self):
        """(packed W * gamma, its row sums, W beta + bias) of ops.outer_fold, cached with the weights."""
        lnm, lin = self.to_out[0], self.to_out[1]
        return self.cached("outer_fold", lambda: ops.outer_fold(lin.weight.detach(), lnm.weight.detach(),
                                                                 lnm.bias.detach(), lin.bias.detach()))

    def run_into(self, x_t, y_t, ln2, feat, feat_ld):
        """Fused form with the consumer's LayerNorm (PairUpdateWithMsa.ln_coevol_feat) in the epilogue: writes 16-bit
        feat[..., 0:288] directly; neither the 1024-wide tensor nor the fp32 result exists.  x_t may be a block of rows
        [B, h, P, N] against y_t [B, L, P, N] (feat [B, h, L, feat_ld])."""
        wp, s_, c_ = self._fold()
        x_t, y_t = self._fused_operands(x_t, y_t)
        return ops.outer_fused(x_t, y_t, wp, s_, c_, None, self.to_out[0].eps,
                               ln2=(_f(ln2.weight), _f(ln2.bias), ln2.eps, feat, feat_ld))

    def run(self, x_t, y_t, N, tape=None):
        """x_t, y_t: T [B, L, P, N] (MSA depth contiguous).  -> fp32 [B,L,L,out].  tape: a dict that receives what _backward
        needs (the two operands; same kernels, same numbers)."""
        B, Lr, P, _ = x_t.shape
        PP = P * P
        lnm = self.to_out[0]
        lin = self.to_out[1]
        _check_backward_call(self, tape, None, PP, lin.weight.shape[0])
        if tape is not None:
            tape.update(x_t=x_t, y_t=y_t)
        if self.fused_ok(P, N, Lr):
            # one kernel: outer product over the MSA depth -> LayerNorm(1024) (folded algebraically) -> Linear; the 1024-wide
            # tensor never leaves the chip (csrc/outer.hip)
            wp, s_, c_ = self._fold()
            out = torch.empty(B, Lr, Lr, lin.weight.shape[0], device=x_t.device, dtype=F32)
            x_t, y_t = self._fused_operands(x_t, y_t)
            return ops.outer_fused(x_t, y_t, wp, s_, c_, out, lnm.eps)
        co = torch.empty(B, Lr, Lr, PP, device=x_t.device, dtype=T())
        if ops.is_h16(T()) and P == 32 and (Lr * P) % 256 == 0 and N >= 64 and RT.fused_outer_ln:
            # LayerNorm(1024) of every pair's outer-product block inside the GEMM epilogue (fp32 statistics on the
            # accumulators): the separate pass over the 0.5 GB feature tensor disappears
            ops.gemm(x_t, y_t, co, Lr * P, Lr * P, N, batch=(B, 1, 1), a_bs=(Lr * P * N, 0, 0), b_bs=(Lr * P * N, 0, 0),
                     c_bs=(Lr * Lr * PP, 0, 0), c_row=(P, Lr * PP, P), c_col=(P, PP), act=L.ACT_BLOCK_LN32,
                     block_ln=(_f(lnm.weight), _f(lnm.bias), lnm.eps))
            cn = co
        else:
            ops.gemm(x_t, y_t, co, Lr * P, Lr * P, N, batch=(B, 1, 1), a_bs=(Lr * P * N, 0, 0), b_bs=(Lr * P * N, 0, 0),
                     c_bs=(Lr * Lr * PP, 0, 0), c_row=(P, Lr * PP, P), c_col=(P, PP))
            cn = ln(lnm, co)
        return ops.linear(cn, self.wt("w", self.to_out[1]), _f(self.to_out[1].bias), out_dtype=F32)

    def run_rows(self, x_rows_t, y_t, N):
        """x_rows_t: T [B, h, P, N] (a block of rows), y_t: T [B, L, P, N] -> fp32 [B, h, L, out]: run() on a rectangular
        block (pair-track row-block sharding), through the fused kernel where run() would take it (the same bits as those
        rows of run(): a pair's result depends on its own operand rows only), else the general path in slabs."""
        _check_backward_call(self, None, "rows")   # a block of rows IS the row-sharded call: refused while recording
        B, h, P, _ = x_rows_t.shape
        Lr = y_t.shape[1]
        PP = P * P
        lnm = self.to_out[0]
        out = torch.empty(B, h, Lr, self.to_out[1].weight.shape[0], device=x_rows_t.device, dtype=F32)
        if self.fused_ok(P, N, Lr):
            wp, s_, c_ = self._fold()
            x_rows_t, y_t = self._fused_operands(x_rows_t, y_t)
            return ops.outer_fused(x_rows_t, y_t, wp, s_, c_, out, lnm.eps)
        # in slabs of rows: the P*P-wide intermediate of a slab stays under 2^28 elements (rf_gemm rejects the 512 x 1024 block of a
        # two-rank split at L = 1024 in one piece; the slab also bounds the 0.5 GB-per-256-rows intermediate)
        step = max(1, (1 << 28) // (Lr * PP * B))
        for i0 in range(0, h, step):
            hs = min(step, h - i0)
            co = torch.empty(B, hs, Lr, PP, device=x_rows_t.device, dtype=T())
            for b in range(B):
                ops.gemm(x_rows_t[b, i0:i0 + hs], y_t[b], co[b], hs * P, Lr * P, N, c_row=(P, Lr * PP, P), c_col=(P, PP))
            y = ops.linear(ln(lnm, co), self.wt("w", self.to_out[1]), _f(self.to_out[1].bias), out_dtype=F32)
            ops.copy(y, out[:, i0:i0 + hs])
        return out

    def forward(self, x, y=None):
        if _recording(self):
            return _RecordedFn.apply(self, x, y, *self.parameters())
        return self._record(x, y, None)

    def _record(self, x, y, tape):
        if tape is not None:
            tape.update(n=x.shape[1], one=y is None)
        B, N, Lr, P = x.shape
        return self.run(*ops.outer_operands(x, x if y is None else y, T(), self.depth_multiple(P, N, Lr)), tape=tape)

    def backward_slab_rows(self, Lr, P):
        """pair rows per slab of _backward: the slab's three P^2-wide tensors stay under RT.outer_bwd_slab_bytes"""
        return max(1, min(Lr, RT.outer_bwd_slab_bytes // (3 * Lr * P * P * (2 if ops.is_h16(T()) else 4))))

    def _backward_from_autograd(self, tape, gs, s, want):
        g = gs[0] if gs[0].dtype == F32 and gs[0].is_contiguous() else gs[0].float().contiguous()
        one = tape["one"]
        (dx, dy), grads = self._backward(tape, g, s, want_x=want[0], want_y=want[1] or (one and want[0]))
        B, Lr, P, _ = tape["x_t"].shape
        N = tape["n"]
        if one and dx is not None:
            ops.axpby(dx, 1.0, dy, 1.0, dx)
            dy = None
        out = []
        for d in (dx, dy):   # T-layout [B, L, P, Np] -> [B, N, L, P] (the inverse of ops.outer_operands), scale taken off
            if d is None:
                out.append(None)
                continue
            _unscale([d], s)
            dn = torch.empty(B, N, Lr, P, device=d.device, dtype=F32)
            ops.copy(d[..., :N], dn.permute(0, 2, 3, 1))
            out.append(dn)
        return tuple(out), grads

    def _backward(self, tape, g, s=1.0, want_x=True, want_y=True):
        """g: contiguous fp32 [B, L, L, out] gradient of the output (read only), s: the factor its 16-bit copies carry (the fp16
        mode's scale).  Returns ((dx_t, dy_t) fp32 [B, L, P, Np] in the operands' transposed layout or None, {param: grad}), all
        still times s.  Per sample and slab of rows i (no [B, L, L, P^2] tensor exists; every sum over slabs is an fp32 addition
        in slab order):
            o  = x_t[i] y_t^T                      rf_gemm, as the general forward writes it
            dz = g W                               rf_gemm
            do, z = LayerNorm backward / forward   rf_layernorm_bwd_fused, in place on dz / o; dgamma, dbeta accumulate
            dW += g^T z, db += sum g               rf_conv_wgrad
            dx_t[i] = do y, dy_t += do^T x[i]      rf_gemm (K chunked over the pair row; do transposed by rf_copy4d for dy)"""
        x_t, y_t = tape["x_t"], tape["y_t"]
        B, Lr, P, Np = x_t.shape
        PP, dev, t = P * P, x_t.device, T()
        lnm, lin = self.to_out[0], self.to_out[1]
        Do = lin.weight.shape[0]
        wt = self.wt_input_grad("w", lin)   # [P^2, out]
        gamma, beta = _f(lnm.weight), _f(lnm.bias)
        h = self.backward_slab_rows(Lr, P)
        # the 16-bit GEMMs take 8-element pieces: with P % 8 the pair row's (j, v) / (i, u) runs are re-laid K-contiguous and
        # zero-padded; otherwise dx reads do in place (K in chunks of P)
        direct = t == F32 or P % 8 == 0
        Kx = pad8(Lr * P)
        co = torch.empty(h, Lr, PP, device=dev, dtype=t)
        dz = torch.empty(h, Lr, PP, device=dev, dtype=t)
        gt = torch.empty(h, Lr, Do, device=dev, dtype=t)
        dgamma = ops.zeros(PP, device=dev, dtype=F32)   # (the slabs' column sums are added to them)
        dbeta = ops.zeros(PP, device=dev, dtype=F32)
        dW = db = None
        dx_t = torch.empty(B, Lr, P, Np, device=dev, dtype=F32) if want_x else None
        dy_t = torch.empty(B, Lr, P, Np, device=dev, dtype=F32) if want_y else None
        first = True
        for b in range(B):
            if want_x:   # y as [Np, (j, v)]: the B operand of dx
                y_n = (ops.zeros if Kx != Lr * P else torch.empty)(Np, Kx, device=dev, dtype=t)
                ops.copy(y_t[b], y_n[:, :Lr * P].unflatten(1, (Lr, P)).permute(1, 2, 0))
            for i0 in range(0, Lr, h):
                hs = min(h, Lr - i0)
                o_s, d_s, g_s = co[:hs], dz[:hs], gt[:hs]
                ops.gemm(x_t[b, i0:i0 + hs], y_t[b], o_s, hs * P, Lr * P, Np, c_row=(P, Lr * PP, P), c_col=(P, PP), exact=True)
                ops.axpby(g[b, i0:i0 + hs], s, None, 0.0, g_s)
                ops.linear(g_s, wt, None, out=d_s, exact=True)
                if RT.outer_bwd_fused:
                    ops.layernorm_bwd_fused(o_s, d_s, gamma, beta, eps=lnm.eps, dx=d_s, z=o_s, dgamma=dgamma, dbeta=dbeta)
                    z_s = o_s
                else:   # the same step on the older engines (A/B timing): three passes and two fp32 copies of the slab
                    z_s = ln(lnm, o_s)
                    do32, dg_s, dbt_s = ops.layernorm_bwd(ops.cast(o_s, F32), ops.cast(d_s, F32), gamma, eps=lnm.eps)
                    ops.axpby(do32, 1.0, None, 0.0, d_s)
                    ops.axpby(dgamma, 1.0, dg_s, 1.0, dgamma)
                    ops.axpby(dbeta, 1.0, dbt_s, 1.0, dbeta)
                dw_s, db_s = ops.conv_wgrad(g_s, z_s, 1, bias=True)
                if first:
                    dW, db = dw_s, db_s
                else:
                    ops.axpby(dW, 1.0, dw_s, 1.0, dW)
                    ops.axpby(db, 1.0, db_s, 1.0, db)
                first = False
                if want_x:
                    c = dx_t[b, i0:i0 + hs]
                    if direct:
                        ops.gemm(d_s, y_n, c, hs * P, Np, Lr * P, kc=P, a_row=(P, Lr * PP, P), a_ko=PP, b_row=(0, 0, Kx), b_ko=P,
                                 exact=True)
                    else:
                        a = ops.zeros(hs * P, Kx, device=dev, dtype=t)
                        ops.copy(d_s.view(hs, Lr, P, P), a.view(hs, P, Kx)[..., :Lr * P].unflatten(2, (Lr, P)).permute(0, 2, 1, 3))
                        ops.gemm(a, y_n, c, hs * P, Np, Kx, exact=True)
                if want_y:   # do^T [(j, v), (i, u)] and x[i] as [Np, (i, u)]
                    Ky = pad8(hs * P)
                    mk = ops.zeros if Ky != hs * P else torch.empty
                    a, x_n = mk(Lr * P, Ky, device=dev, dtype=t), mk(Np, Ky, device=dev, dtype=t)
                    ops.copy(d_s.view(hs, Lr, P, P), a.view(Lr, P, Ky)[..., :hs * P].unflatten(2, (hs, P)).permute(2, 0, 3, 1))
                    ops.copy(x_t[b, i0:i0 + hs], x_n[:, :hs * P].unflatten(1, (hs, P)).permute(1, 2, 0))
                    ops.gemm(a, x_n, dy_t[b], Lr * P, Np, Ky, residual=dy_t[b] if i0 else None, exact=True)
        return (dx_t, dy_t), {lin.weight: dW, lin.bias: db, lnm.weight: dgamma, lnm.bias: dbeta}


class PairUpdateWithMsa(RFModule):
    """rf.py:430-498."""

    def __init__(self, d_msa, d_proj, d_pair, n_heads, p_dropout=0.1):
        super().__init__()
        self.d_proj, self.d_pair, self.n_heads = d_proj, d_pair, n_heads
        self.proj_msa = nn.Sequential(LayerNorm(d_msa), Linear(d_msa, d_proj), LayerNorm(d_proj))
        self.poswise_weight = PositionWiseWeightFactor(d_proj, 1, p_dropout)
        self.outer_product_mean = OuterProductMean(d_proj, d_pair)
        self.ln_coevol_feat = LayerNorm(d_pair)
        self.ln_pair = LayerNorm(d_pair)
        d_feat_full = d_pair * 2 + d_proj * 4 + n_heads
        self.d_feat = d_feat_full
        self.resnet = nn.Sequential(
            Linear(d_feat_full, d_pair),
            Residual(nn.Sequential(
                nn.Identity(),
                nn.Conv2d(d_pair, d_pair, kernel_size=3, padding="same", bias=False),
                nn.InstanceNorm2d(d_pair, affine=True, eps=1e-6),
                nn.ELU(),
                nn.Dropout(p_dropout),
                nn.Conv2d(d_pair, d_pair, kernel_size=3, padding="same", bias=False),
                nn.InstanceNorm2d(d_pair, affine=True, eps=1e-6),
                nn.Identity(),
            )),
            nn.ELU(),
        )

    def _msa_operands(self, msa):
        """Per-position features of the MSA: (msa1d fp32 [B,L,2P], x_t, y_t T [B,L,P,Np] = the transposed operands of the outer
        product, Np)."""
        B, N, Lr, D = msa.shape
        P = self.d_proj
        dev = msa.device
        mp_pre = ops.linear(ln(self.proj_msa[0], msa), self.wt("p", self.proj_msa[1]), _f(self.proj_msa[1].bias),
                            out_dtype=F32)
        mp = ln(self.proj_msa[2], mp_pre)  # T [B,N,L,P]
        w = self.poswise_weight.weights(mp)  # fp32 [B,N,1,L]
        # 1-D features: sum over N and the query row
        msa1d = torch.empty(B, Lr, 2 * P, device=dev, dtype=F32)
        ones = ops.fill(torch.empty(B, N, 1, Lr, device=dev, dtype=F32), 1.0)
        ops.weighted_msa_sum(mp, ones, msa1d, 2 * P)
        ops.copy(mp[:, 0], msa1d[..., P:])
        # transposed operands of the outer product: x_t[b,i,u,n] = mp ; y_t = mp * w   (rf.py:472-473)
        mpw = ops.scale_rows(mp, w, B * N * Lr, P)
        return (msa1d,) + ops.outer_operands(mp, mpw, T(), self.outer_product_mean.depth_multiple(P, N, Lr))

    # ---- operand conditioning of the 16-bit modes (csrc/condition.hip; tools/precision_probe.py --pum-sweep) ------------------
    # At random init the 1-D features and the projected feature tensor are a per-sample constant plus a part ~20x smaller that
    # varies over the picture, and the ResNet's InstanceNorms keep only the latter: rounded to 16 bits WITH the constant, the
    # tiled 1-D features (1.3e-2), the first convolution's input (9.7e-3) and its output (7.3e-3) were 1.8e-2 of the fp16 mode's
    # 2.0e-2 logits gap at the benchmarked depth.  Both constants are removed before the rounding and carried in fp32:
    #   W (f - m) + (b + W m) == W f + b                           (the 1-D features' mean through the projection's bias)
    #   conv3x3(x - c) + [border terms] == conv3x3(x) - sum_taps W_tap c   (a per-channel constant: the InstanceNorm drops it)
    def _center_1d(self, msa1d, bias):
        P, Dp = self.d_proj, self.d_pair
        w32 = self.cached("f_f32", lambda: self.resnet[0].weight.detach().float().contiguous())
        return ops.fold_mean(w32, ops.center_rows(msa1d), bias, k0=Dp, nseg=2, seg_stride=2 * P)

    def _conv_taps(self, conv, cx):
        Co, Ci = conv.weight.shape[:2]
        w32 = self.cached("c1_f32", lambda: conv.weight.detach().permute(0, 2, 3, 1).reshape(Co, 9 * Ci).float().contiguous())
        return ops.fold_mean(w32, cx, None, nseg=9, seg_stride=Ci, sum_seg=False)   # [B, 9, Co]

    def run_rows(self, msa, pair_rows, att, row_group):
        """run() for a block of pair rows (pair-track row-block sharding, shard.pair_update_with_msa_row_sharded): msa
        [B,N,L,D] and att [B,L,L,H] are replicated, pair_rows fp32 [B,h,L,Dp] are this rank's rows shard_range(L, world, rank).
        The outer product, the feature assembly and the projection are local to the rows; the two 3x3 convolutions fetch one
        halo row from each neighbour and the two InstanceNorms all-reduce their sums.  Returns the new rows (fp32)."""
        from . import shard
        B, N, Lr, D = msa.shape
        P, Dp = self.d_proj, self.d_pair
        dev = msa.device
        h = pair_rows.shape[1]
        r0, r1 = shard.shard_range(Lr, shard.group_size(row_group), shard.group_rank(row_group))
        if r1 - r0 != h or h == 0:
            raise ValueError(f"pair rows {h} do not match this rank's (non-empty) share {r1 - r0} of {Lr}")
        msa1d, xt, yt, Np = self._msa_operands(msa)
        Kf = pad8(self.d_feat)
        feat = ops.zeros(B, h, Lr, Kf, device=dev, dtype=T())
        # outer product of this block's rows with every column: the fused kernel on the rectangle, as run() does on the square
        xr = ops.copy(xt[:, r0:r1], torch.empty(B, h, P, Np, device=dev, dtype=T()))
        if self.outer_product_mean.fused_ok(P, Np, Lr) and Dp == 288:
            self.outer_product_mean.run_into(xr, yt, self.ln_coevol_feat, feat, Kf)  # -> feat[..., :Dp]
        else:
            coevol = self.outer_product_mean.run_rows(xr, yt, Np)  # fp32 [B,h,L,Dp]
            ln(self.ln_coevol_feat, coevol, out=feat, out_ld=Kf, out_off=0)
        cond = RT.condition and ops.is_h16(T()) and Dp % 4 == 0   # (rf_center_apply moves 16-byte chunks of a pixel)
        bias = _f(self.resnet[0].bias)
        if cond:   # (the mean over ALL positions: msa is replicated, every rank folds the same constant)
            bias_b = self._center_1d(msa1d, bias)
        # feat[b,i,j, Dp + c] = msa1d[b, r0 + i, c] ; feat[b,i,j, Dp + 2P + c] = msa1d[b, j, c]   (rf_tile_1d_feats on a block)
        ops.copy(msa1d[:, r0:r1, None, :].expand(B, h, Lr, 2 * P), feat[..., Dp:Dp + 2 * P])
        ops.copy(msa1d[:, None, :, :].expand(B, h, Lr, 2 * P), feat[..., Dp + 2 * P:Dp + 4 * P])
        ln(self.ln_pair, pair_rows, out=feat, out_ld=Kf, out_off=Dp + 4 * P)
        H = att.shape[-1]
        ops.copy(att[:, r0:r1], feat[..., 2 * Dp + 4 * P:2 * Dp + 4 * P + H])
        blk = self.resnet[1].fn
        kw = {"row_group": row_group, "rows_global": Lr}
        if cond:
            x = torch.empty(B, h, Lr, Dp, device=dev, dtype=F32)
            for b in range(B):
                ops.linear(feat[b], self.wt("f", self.resnet[0], kpad=Kf), bias_b[b], out=x[b])
            cx = ops.channel_mean(x, **kw)
            taps = self._conv_taps(blk[1], cx)
            n_r, r_ = shard.group_size(row_group), shard.group_rank(row_group)
            edges = 12 | (1 if r_ == 0 else 0) | (2 if r_ == n_r - 1 else 0)   # left | right, top / bottom on the outer ranks
        else:
            x = ops.linear(feat, self.wt("f", self.resnet[0], kpad=Kf), bias, out_dtype=F32)
        if B == 1:   # one picture: pre-haloed buffers, only the halo rows move (see ResBlock2D._run_rows_b1)
            xh = shard.haloed_buffer(h, Lr, Dp, 1, dev, T())
            if cond:
                ops.center_apply(x, cx, out=shard.interior(xh, 1))
            else:
                ops.axpby(x, 1.0, None, 0.0, shard.interior(xh, 1))
            shard.exchange_row_halos_inplace(xh, 1, row_group)
            y = conv3x3(self, "c1", blk[1], xh, 1)
            if cond:
                ops.conv3x3_border_fix(shard.interior(y, 1), taps, 1, edges)
            yh = shard.haloed_buffer(h, Lr, Dp, 1, dev, T())
            ops.instnorm(shard.interior(y, 1), _f(blk[2].weight), _f(blk[2].bias), eps=blk[2].eps, act=L.ACT_ELU,
                         out=shard.interior(yh, 1), **kw)
            shard.exchange_row_halos_inplace(yh, 1, row_group)
            y = conv3x3(self, "c2", blk[5], yh, 1)
            out, _ = ops.instnorm(shard.interior(y, 1), _f(blk[6].weight), _f(blk[6].bias), eps=blk[6].eps, residual=x,
                                  act=L.ACT_ELU, out_dtype=F32, **kw)
            return out
        conv = lambda key, c, t: shard.drop_row_halos(conv3x3(self, key, c, shard.exchange_row_halos(t, 1, row_group), 1), 1)  # noqa: E731
        if cond:
            y = ops.conv3x3_border_fix(conv("c1", blk[1], ops.center_apply(x, cx, out_dtype=T())), taps, 1, edges)
        else:
            y = conv("c1", blk[1], ops.cast(x, T()))
        y, _ = ops.instnorm(y, _f(blk[2].weight), _f(blk[2].bias), eps=blk[2].eps, act=L.ACT_ELU, out_dtype=T(), **kw)
        y = conv("c2", blk[5], y)
        out, _ = ops.instnorm(y, _f(blk[6].weight), _f(blk[6].bias), eps=blk[6].eps, residual=x, act=L.ACT_ELU,
                              out_dtype=F32, **kw)
        return out

    def run(self, msa, pair, att):
        """msa fp32 [B,N,L,D], pair fp32 [B,L,L,Dp], att fp32 [B,L,L,H] -> new pair fp32."""
        B, N, Lr, D = msa.shape
        P, Dp = self.d_proj, self.d_pair
        dev = msa.device
        msa1d, xt, yt, Np = self._msa_operands(msa)
        # feature tensor (K padded to a multiple of 8)
        Kf = pad8(self.d_feat)
        feat = torch.empty(B, Lr, Lr, Kf, device=dev, dtype=T())  # every feature column is written below; only the K padding
        if Kf > self.d_feat:                                       # needs zeros (a full memset of this tensor is 0.38 GB)
            ops.copy(ops.zeros(B, Lr, Lr, Kf - self.d_feat, device=dev, dtype=T()), feat[..., self.d_feat:])
        if self.outer_product_mean.fused_ok(P, Np, Lr) and Dp == 288:
            self.outer_product_mean.run_into(xt, yt, self.ln_coevol_feat, feat, Kf)  # outer -> LN -> Linear -> LN -> feat[..., :Dp]
        else:
            coevol = self.outer_product_mean.run(xt, yt, Np)  # fp32 [B,L,L,Dp]
            ln(self.ln_coevol_feat, coevol, out=feat, out_ld=Kf, out_off=0)
        H = att.shape[-1]
        blk = self.resnet[1].fn
        cond = RT.condition and ops.is_h16(T()) and Dp % 4 == 0   # (rf_center_apply moves 16-byte chunks of a pixel)
        bias = _f(self.resnet[0].bias)
        if cond:
            bias_b = self._center_1d(msa1d, bias)   # msa1d -= its mean over the positions; [B, Dp] bias that carries W * mean
        ops.tile_1d_feats(msa1d, feat, Kf, Dp, B, Lr, 2 * P)
        ln(self.ln_pair, pair, out=feat, out_ld=Kf, out_off=Dp + 4 * P)
        ops.copy(att, feat[..., 2 * Dp + 4 * P:2 * Dp + 4 * P + H])
        if cond:
            x = torch.empty(B, Lr, Lr, Dp, device=dev, dtype=F32)
            for b in range(B):
                ops.linear(feat[b], self.wt("f", self.resnet[0], kpad=Kf), bias_b[b], out=x[b])
            cx = ops.sample_mean(x)   # an estimate serves: both identities hold for ANY constant (a row-sharded picture needs the
            #                           same constant on every rank: run_rows all-reduces the exact mean)
            y = conv3x3(self, "c1", blk[1], ops.center_apply(x, cx, out_dtype=T()), 1)
            ops.conv3x3_border_fix(y, self._conv_taps(blk[1], cx), 1)
        else:
            x = ops.linear(feat, self.wt("f", self.resnet[0], kpad=Kf), bias, out_dtype=F32)
            y = conv3x3(self, "c1", blk[1], ops.cast(x, T()), 1)
        y, _ = ops.instnorm(y, _f(blk[2].weight), _f(blk[2].bias), eps=blk[2].eps, act=L.ACT_ELU, out_dtype=T())
        if self.training:
            dropout_(y, _p(blk[4]))   # rf.py:455
        y = conv3x3(self, "c2", blk[5], y, 1)
        out, _ = ops.instnorm(y, _f(blk[6].weight), _f(blk[6].bias), eps=blk[6].eps, residual=x, act=L.ACT_ELU,
                              out_dtype=F32)
        return out

    def forward(self, msa, pair, att):
        return self.run(msa.float().contiguous(), pair.float().contiguous(), att.float().contiguous())


def conv3x3(mod, key, conv, x, dilation, out_dtype=None):
    """3x3 'same' convolution on NHWC x (T) as implicit GEMM (rf.py:452,456; resnet.py:19-38)."""
    B, Hh, Ww, Cc = x.shape
    Co = conv.weight.shape[0]
    wk = mod.cached(("conv", key), lambda: conv.weight.detach().permute(0, 2, 3, 1).reshape(Co, 9 * Cc).to(T()).contiguous())
    out = torch.empty(B, Hh, Ww, Co, device=x.device, dtype=out_dtype or T())
    ops.gemm(x, wk, out, B * Hh * Ww, Co, 9 * Cc, conv=(B, Hh, Ww, Cc, dilation),
             bias=_f(conv.bias) if conv.bias is not None else None)
    return out


# ================================================================================================
# pair axial attention
# ================================================================================================
class PairUpdateWithAxialAttentionLayer(RecordingModule):
    """rf.py:501-528.  RowWise: sequences along dim 1 (i) for fixed j; ColWise: along dim 2 (rf.py:31-54).
    enable_backward(): the layer, its two Performers and its FeedForward."""
    _rf_scales_own_grads = True   # per sub-layer: _pre_norm_residual_bwd

    def __init__(self, d_pair, d_ff, n_heads, p_dropout, performer_kws):
        super().__init__()
        self.row_attn = PerformerSelfAttention(dim=d_pair, heads=n_heads, dropout=p_dropout,
                                               generalized_attention=True, **performer_kws)
        self.col_attn = PerformerSelfAttention(dim=d_pair, heads=n_heads, dropout=p_dropout,
                                               generalized_attention=True, **performer_kws)
        self.ff = FeedForward(d_pair, d_ff, p_dropout)
        # same aliasing as the reference: layer.k.fn.0 = LayerNorm, layer.0.fn.1.fn = row_attn, ...
        self.layer = nn.Sequential(
            Residual(nn.Sequential(LayerNorm(d_pair), RowWise(self.row_attn))),
            Residual(nn.Sequential(LayerNorm(d_pair), ColWise(self.col_attn))),
            Residual(nn.Sequential(LayerNorm(d_pair), self.ff)),
        )

    def run(self, x, xn=None, next_ln=None, row_group=None, tape=None):
        """x fp32 in place; xn = layer[0] pre-norm of x if already produced; returns next_ln(x) or None.
        row_group: x holds a block of ROWS (dim 1) of the pair tensor, the other row blocks live on the other ranks of this
        torch.distributed group (shard.pair_axial_layer_row_sharded): the RowWise attention all-reduces its contexts, the
        ColWise attention and the feed-forward are local.
        tape: a dict that receives what _backward needs (an fp32 copy of x in front of each sub-layer -- x is updated in place
        -- and the sub-layers' tapes); the kernels and numbers are those of the plain call."""
        l0, l1, l2 = self.layer[0].fn[0], self.layer[1].fn[0], self.layer[2].fn[0]
        _check_backward_call(self, tape, row_group, x.shape[-1])
        if tape is not None:
            tape.update(row={}, col={}, ff={})
        snap = (lambda k: tape.__setitem__(k, _copy(x))) if tape is not None else (lambda k: None)
        if row_group is not None and RT.rowshard_attention == "transpose":
            # the direction that crosses the row blocks, on the TRANSPOSED blocks: two transposing exchanges of the fp32 stream
            # (1/world of the tensor per rank each) instead of the all-reduce of the contexts (0.57 GB per rank at L = 1024 whatever
            # the world size), and every sequence is whole on its rank again -- the fused FAVOR+ kernel runs as in one process
            from . import shard
            xt = shard.transpose_row_sharded(x, row_group)
            self.row_attn.attend(ln(l0, xt), xt, axis=2)
            ops.axpby(shard.transpose_row_sharded(xt, row_group), 1.0, None, 0.0, x)
            xn = None
        else:
            if xn is None:
                xn = ln(l0, x)
            snap("x0")
            xn = self.row_attn.attend(xn, x, axis=1, next_ln=l1, seq_group=row_group,
                                      drops=(self.row_attn.p_dropout,) if self.training else (),
                                      tape=tape["row"] if tape is not None else None)
        if xn is None:
            xn = ln(l1, x)
        snap("x1")
        xn = self.col_attn.attend(xn, x, axis=2, next_ln=l2, drops=(self.col_attn.p_dropout,) if self.training else (),
                                  tape=tape["col"] if tape is not None else None)
        if xn is None:
            xn = ln(l2, x)
        snap("x2")
        # (its hidden dropout, rf.py:519, is the FeedForward's own)
        return self.ff.apply_residual(xn, x, next_ln, tape=tape["ff"] if tape is not None else None)

    def _backward(self, tape, g):
        """g: fp32 gradient of the layer's output (overwritten).  Returns (fp32 gradient of its input, {param: grad})."""
        grads = {}
        _pre_norm_residual_bwd(g, self.ff._backward, tape["ff"], tape["x2"], self.layer[2].fn[0], grads)
        _pre_norm_residual_bwd(g, self.col_attn._backward, tape["col"], tape["x1"], self.layer[1].fn[0], grads)
        _pre_norm_residual_bwd(g, self.row_attn._backward, tape["row"], tape["x0"], self.layer[0].fn[0], grads)
        return g, grads

    def _backward_children(self):
        return self.row_attn, self.col_attn, self.ff

    def _record(self, x, tape):
        x = fresh_f32(x)
        self.run(x, tape=tape)
        return x


class PairUpdateWithAxialAttention(RecordingModule):
    """rf.py:531-547.  enable_backward(): the stack and every layer below it (see PairUpdateWithAxialAttentionLayer).  Inside
    RoseTTAFold.forward only the final block's stack records, and only together with the prediction head."""
    _rf_scales_own_grads = True
    _record = PairUpdateWithAxialAttentionLayer._record

    def __init__(self, d_pair, d_ff, n_heads, p_dropout, n_encoder_layers, performer_kws={}):
        super().__init__()
        self.layers = nn.ModuleList([PairUpdateWithAxialAttentionLayer(d_pair, d_ff, n_heads, p_dropout, performer_kws)
                                     for _ in range(n_encoder_layers)])

    def run(self, x, row_group=None, tape=None):
        """x fp32 in place.  tape: a dict that receives the layers' tapes (see PairUpdateWithAxialAttentionLayer.run)."""
        _check_backward_call(self, tape, row_group, x.shape[-1])
        if tape is not None:
            tape["layers"] = [{} for _ in self.layers]
        xn = None
        for i, layer in enumerate(self.layers):
            nxt = self.layers[i + 1].layer[0].fn[0] if i + 1 < len(self.layers) else None
            xn = layer.run(x, xn=xn, next_ln=nxt, row_group=row_group, tape=tape["layers"][i] if tape is not None else None)

    def _backward(self, tape, g):
        grads = {}
        for i in reversed(range(len(self.layers))):
            g, gr = self.layers[i]._backward(tape["layers"][i], g)
            grads.update(gr)
        return g, grads

    def _backward_children(self):
        return self.layers


# ================================================================================================
# MSA update with pair
# ================================================================================================
class Symmetrization(nn.Module):
    """rf.py:550-556 (container; the arithmetic is fused into rf_sym_layernorm)."""

    def forward(self, x):
        xt = torch.empty_like(x)
        ops.copy(x.transpose(1, 2), xt)
        return ops.axpby(x.contiguous(), 0.5, xt, 0.5, torch.empty_like(x))


class MsaUpdateWithPairLayer(RecordingModule):
    """rf.py:559-595.  enable_backward() (switches the FeedForward in `ff` along): with grad mode on, forward(msa, pair) records,
    and loss.backward() fills the .grad of every parameter of the layer and of msa and pair where they require grad (the
    backward: MsaUpdateWithPair._backward, on a stack of this one layer).  MsaUpdateWithPair.run calls run() with the stack's
    tape or with none; the trunk never hands one in."""
    _rf_n_inputs = 2
    _rf_scales_own_grads = True

    def __init__(self, d_msa, d_pair, n_heads, p_dropout=0.1):
        super().__init__()
        self.n_heads = n_heads
        self.pair2att = nn.Sequential(Symmetrization(), LayerNorm(d_pair), Linear(d_pair, n_heads),
                                      nn.Dropout(p_dropout), nn.Identity(), nn.Softmax(dim=-1))
        self.msa2value = nn.Sequential(LayerNorm(d_msa), Linear(d_msa, d_msa), nn.Identity())
        self.ff = Residual(nn.Sequential(LayerNorm(d_msa), FeedForward(d_msa, d_msa, p_dropout)), p_dropout=p_dropout)
        self.p_dropout = p_dropout   # rf.py:586,592: dropout on the attention output before it is added to the msa

    def folded_att_proj(self):
        """LayerNorm affine folded into the 288->H projection: W' = W*gamma, b' = W beta + b (fp32)."""
        lnm, lin = self.pair2att[1], self.pair2att[2]
        w = lin.weight.detach().float() * lnm.weight.detach().float()[None, :]
        b = lin.weight.detach().float() @ lnm.bias.detach().float() + lin.bias.detach().float()
        return w, b

    def run(self, msa, att, xn=None, next_ln=None, row_group=None, tape=None):
        """msa fp32 [B,N,L,D] in place; att: T [H,B,L,L] (softmax over the last dim); xn = msa2value pre-norm if the
        previous GEMM produced it; returns next_ln(msa) or None.
        row_group: att holds this rank's rows [H,B,h,L] of the maps (pair-track row blocks, shard.shard_range); the values are
        computed from the replicated msa, positions r0..r1 are updated here (attention + feed-forward) and the updated position
        slices are all-gathered so that msa is whole again on every rank.
        tape: a dict that receives what the backward needs (an fp32 copy of msa in front of the attention and in front of the
        feed-forward -- msa is updated in place --, the attention-output dropout's records and the feed-forward's tape); the
        kernels and numbers are those of the plain call."""
        D = msa.shape[-1]
        _check_backward_call(self, tape, row_group, D, D // self.n_heads)
        if row_group is not None:
            return self._run_rows(msa, att, xn, row_group)
        v_t = self._values(msa, xn)
        sub = None
        if tape is not None:
            sub = {}
            tape.update(x0=_copy(msa), att_drops=[], ff=sub)
        drops = ()
        if self.training and self.p_dropout and self.p_dropout > 0:
            add_dropped(msa, lambda tmp: self._add_attention_values(att, v_t, tmp), (self.p_dropout,),
                        tape["att_drops"] if tape is not None else None)
            drops = (self.ff.p_dropout,)
        else:
            self._add_attention_values(att, v_t, msa)
        if tape is not None:
            tape["x1"] = _copy(msa)
        return self._feed_forward(msa, next_ln, drops=drops, tape=sub)

    def _run_rows(self, msa, att, xn, row_group):
        """run() for a block of map rows (see there)."""
        from . import shard
        B, N, Lr, D = msa.shape
        h = att.shape[2]
        r0, r1 = shard.shard_range(Lr, shard.group_size(row_group), shard.group_rank(row_group))
        if r1 - r0 != h:
            raise ValueError(f"attention rows {h} do not match this rank's share {r1 - r0} of {Lr} positions")
        v_t = self._values(msa, xn)
        rows = torch.empty(B, N, h, D, device=msa.device, dtype=F32)   # msa[:, :, r0:r1]
        if h > 0:
            ops.copy(msa[:, :, r0:r1], rows)
            self._add_attention_values(att, v_t, rows)
            self._feed_forward(rows, None)
        shard.all_gather_positions(rows, msa, row_group)
        return None

    def _values(self, msa, xn):
        """msa2value, key-contiguous: T [B,N,D,L] (xn: its pre-norm if the previous GEMM produced it)."""
        if xn is None:
            xn = ln(self.msa2value[0], msa)
        return self.values_transposed(self.msa2value[1], xn, _f(self.msa2value[1].bias))

    def _add_attention_values(self, att, v_t, dst):
        """dst += att @ v  (rf.py:592-595), scattered back to [b,n,i,(h,d)]: att T [H,B,h,L] (h query rows: all L, or a rank's
        block), v_t T [B,N,D,L], dst fp32 [B,N,h,D].  (L here is the operands' key extent map_ld(L): zero pad columns on both.)"""
        H, B, h, Lr = att.shape
        N, D = v_t.shape[1], v_t.shape[2]
        dv = D // H
        ops.gemm(att, v_t, dst, h, N * dv, Lr, batch=(H, B, 1),
                 a_bs=(B * h * Lr, h * Lr, 0), a_row=(0, 0, Lr),
                 b_bs=(dv * Lr, N * D * Lr, 0), b_row=(dv, D * Lr, Lr),
                 c_bs=(dv, N * h * D, 0), c_row=(0, 0, D), c_col=(dv, h * D), residual=dst)

    def _feed_forward(self, x, next_ln, drops=(), tape=None):
        return self.ff.fn[1].apply_residual(ln(self.ff.fn[0], x), x, next_ln, drops=drops, tape=tape)

    def _backward_layer(self, tape, g, att, datt):
        """The layer's part of MsaUpdateWithPair._backward.  g: fp32 [B,N,L,D] gradient of the layer's output, updated in place
        to the gradient of its msa input; att: the layer's maps T [H,B,L,Lp] as the forward wrote them (Lp = map_ld(L), zero pad
        columns); datt: fp32 [H,B,L,L], receives the maps' gradient at scale 1.  Returns {param: grad}.
        LN(msa), the row-major values and g key-contiguous are rebuilt from the saved stream; the attention . V half runs on a
        copy of g at a power-of-two scale of its own (the fp16 mode), taken off datt, d msa and the parameters in fp32."""
        x0 = tape["x0"]
        B, N, Lr, D = x0.shape
        H, Lp, dev = self.n_heads, att.shape[-1], x0.device
        dv = D // H
        lnv, lin = self.msa2value[0], self.msa2value[1]
        grads = {}
        _pre_norm_residual_bwd(g, self.ff.fn[1]._backward, tape["ff"], tape["x1"], self.ff.fn[0], grads)
        s = _grad_scale([g])
        go = _scaled_copy(g, s)
        for rec in tape["att_drops"]:
            _replay_dropout(go, rec)
        go_t = ops.cast(go, T())
        xn = ln(lnv, x0)
        v = ops.linear(xn, self.wt("v", lin), _f(lin.bias), exact=True)   # the values row-major: [B,N,L,D] T
        ops.gemm(go_t, v, datt, Lr, Lr, N * dv, batch=(H, B, 1), kc=dv,
                 a_bs=(dv, N * Lr * D, 0), a_row=(0, 0, D), a_ko=Lr * D,
                 b_bs=(dv, N * Lr * D, 0), b_row=(0, 0, D), b_ko=Lr * D,
                 c_bs=(B * Lr * Lr, Lr * Lr, 0), c_row=(0, 0, Lr), exact=True)
        del v
        _unscale([datt], s)
        mk = torch.empty if Lp == Lr else ops.zeros
        go_tt = mk(B, N, D, Lp, device=dev, dtype=T())        # g key-contiguous, like the forward's v^T
        ops.copy(go_t.transpose(2, 3), go_tt[..., :Lr])
        att_tr = mk(H, B, Lr, Lp, device=dev, dtype=att.dtype)
        ops.copy(att[..., :Lr].transpose(2, 3), att_tr[..., :Lr])
        del go, go_t
        dv_t = torch.empty(B, N, Lr, D, device=dev, dtype=T())
        ops.gemm(att_tr, go_tt, dv_t, Lr, N * dv, Lp, batch=(H, B, 1),
                 a_bs=(B * Lr * Lp, Lr * Lp, 0), a_row=(0, 0, Lp),
                 b_bs=(dv * Lp, N * D * Lp, 0), b_row=(dv, D * Lp, Lp),
                 c_bs=(dv, N * Lr * D, 0), c_row=(0, 0, D), c_col=(dv, Lr * D), exact=True)
        del att_tr, go_tt
        dwv, dbv = ops.conv_wgrad(dv_t, xn, 1, bias=True)
        dm = ops.linear(dv_t, self.wt_input_grad("v", lin), None, out_dtype=F32, exact=True)
        del dv_t, xn
        gr = {lin.weight: dwv, lin.bias: dbv}
        _unscale([dm] + list(gr.values()), s)
        dx, gr[lnv.weight], gr[lnv.bias] = ops.layernorm_bwd(x0, dm, _f(lnv.weight), eps=lnv.eps)
        ops.axpby(g, 1.0, dx, 1.0, g)
        grads.update(gr)
        return grads

    def _backward(self, tape, g, want_pair=True):
        return _msa_update_with_pair_backward([self], tape, g, want_pair)

    def _backward_children(self):
        return (self.ff.fn[1],)

    def _record(self, msa, pair, tape):
        msa = fresh_f32(msa)
        if tape is not None:
            tape.update(front={}, layers=[{}])
        att = pair_to_att([self], pair.float().contiguous(), tape=tape["front"] if tape is not None else None)[0]
        self.run(msa, att, tape=tape["layers"][0] if tape is not None else None)
        return msa

    def _backward_from_autograd(self, tape, gs, s, want):
        dmsa, dpair, grads = self._backward(tape, _scaled_copy(gs[0], 1.0), want_pair=want[1])
        return (dmsa, dpair), grads

    def forward(self, msa, pair):
        if _recording(self):
            return _RecordedFn.apply(self, msa, pair, *self.parameters())
        return self._record(msa, pair, None)


def _pair_logits(layers, pair, row_group=None):
    """The front of pair_to_att up to the logits: (the symmetrised, normalised pair tensor T [B,h,L,Dp] without the LayerNorm's
    affine, fp32 logits [B,h,L,nl*H] of every layer's heads from the folded projection)."""
    holder = layers[0]
    nl, Dp = len(layers), pair.shape[-1]
    eps = holder.pair2att[1].eps
    if row_group is None:
        xs = ops.sym_layernorm(pair, T(), eps=eps)
    else:
        from . import shard
        xt = shard.transpose_row_sharded(pair, row_group)
        sym = ops.axpby(pair, 0.5, xt, 0.5, torch.empty_like(pair))
        one, zero = ops.fill(torch.empty(Dp, device=pair.device, dtype=F32), 1.0), ops.zeros(Dp, device=pair.device, dtype=F32)
        xs = ops.layernorm(sym, one, zero, eps=eps, out_dtype=T())
    # (neither front applies the LayerNorm's affine: it is folded into the projection)

    def fold():
        ws, bs = zip(*[l.folded_att_proj() for l in layers])
        return torch.cat(ws, 0).to(T()).contiguous(), torch.cat(bs, 0).contiguous()

    wc, bc = holder.cached(("att_fold", nl), fold)
    return xs, ops.linear(xs, wc, bc, out_dtype=F32)


def _pair_maps(logits, nl, H):
    """every (layer, head) softmax in one launch: problem z = li*H + h is column z of the logits [B,h,L,nl*H]
    (16-bit modes: rows Lp = map_ld(L) apart with zeros in the pad columns, the contraction of _add_attention_values runs over Lp)"""
    B, h, Lr, NH = logits.shape
    Lp = map_ld(Lr)
    att_all = (torch.empty if Lp == Lr else ops.zeros)(nl, H, B, h, Lp, device=logits.device, dtype=T())
    if h > 0:
        ops.softmax_batched(logits, 1, Lr * NH, NH, att_all, B * h * Lp, Lp, B * h, Lr, NH)
    return [att_all[li] for li in range(nl)]


def pair_to_att(layers, pair, row_group=None, tape=None):
    """Shared front of the MsaUpdateWithPairLayer stack of one block (they all see the same pair):
    one symmetrise+normalise pass, one GEMM for every layer's head logits, per-(layer,head) softmax.
    Returns a list of T [H,B,L,Lp] ([H,B,h,Lp] for a block of h pair rows: row_group, the transposed sub-blocks of the
    symmetrisation come from the other ranks); Lp = map_ld(L), columns L..Lp are zeros.
    tape: a dict that receives pair and the logit dropout's record (same kernels, same numbers)."""
    holder = layers[0]
    _check_backward_call(holder, tape, row_group, pair.shape[-1])
    _, logits = _pair_logits(layers, pair, row_group)  # [B,h,L,nl*H]
    rec = None
    if holder.training and row_group is None:   # (the row-sharded forward is the inference path: shard.forward_row_sharded)
        p = _p(holder.pair2att[3])   # rf.py:567: Dropout sits between the projection and the softmax
        if tape is None:
            dropout_(logits, p)
        else:
            rec = _dropout_rec(logits, p)
    if tape is not None:
        tape.update(pair=pair, drop=rec)
    return _pair_maps(logits, len(layers), holder.n_heads)


def _msa_update_with_pair_backward(layers, tape, g, want_pair=True):
    """Backward of a stack of MsaUpdateWithPairLayer over one pair tensor (MsaUpdateWithPair._backward; a lone layer is a stack of
    one).  g: contiguous fp32 [B,N,L,D] gradient of the output (overwritten).  Returns (fp32 d msa, fp32 d pair or None,
    {param: grad})."""
    front = tape["front"]
    pair, rec = front["pair"], front["drop"]
    B, Lr, _, Dp = pair.shape
    holder = layers[0]
    H, nl = holder.n_heads, len(layers)
    NZ, dev = nl * H, pair.device
    xs, logits = _pair_logits(layers, pair)
    _replay_dropout(logits, rec)
    atts = _pair_maps(logits, nl, H)
    datt = torch.empty(NZ, B, Lr, Lr, device=dev, dtype=F32)
    grads = {}
    for li in reversed(range(nl)):
        grads.update(layers[li]._backward_layer(tape["layers"][li], g, atts[li], datt[li * H:(li + 1) * H]))
    del atts
    # ---- every map's softmax in one launch; the logit dropout; the folded projection; symmetrise -> LayerNorm
    h16 = ops.is_h16(T())
    nzp = pad8(NZ)
    late = h16 and (rec is not None or T() == torch.float16)   # the 16-bit copy follows the replay and the fp16 scale
    dz, dz16 = ops.pair_softmax_bwd(logits, datt, nz_pad=nzp if h16 and not late else None)
    del logits, datt
    _replay_dropout(dz, rec)
    w32 = holder.cached(("att_fold32", nl), lambda: torch.cat([l.folded_att_proj()[0] for l in layers], 0).contiguous())
    dpair = ops.sym_layernorm_bwd(pair, dz, w32, eps=holder.pair2att[1].eps) if want_pair else None
    s = 1.0
    if late:
        s = _grad_scale([dz])
        if s != 1.0:
            ops.axpby(dz, s, None, 0.0, dz)
        dz16 = (torch.empty if nzp == NZ else ops.zeros)(B, Lr, Lr, nzp, device=dev, dtype=T())
        ops.copy(dz, dz16[..., :NZ])
    dwf, dbf = ops.conv_wgrad(dz16 if h16 else dz, xs, 1, bias=True)   # the folded dW' [>= NZ, Dp], db' [>= NZ]
    del xs, dz, dz16
    _unscale([dwf, dbf], s)
    # ---- unfolded per layer ([H, Dp]): dW = dW' gamma (+ db' beta^T), dgamma = sum_h dW' W (both: rf_scale_rows_bwd over the Dp
    # columns as rows), db = db', dbeta = W^T db'
    for li, layer in enumerate(layers):
        lnm, lin = layer.pair2att[1], layer.pair2att[2]
        wt32 = layer.cached("att_w_t32", lambda: lin.weight.detach().float().t().contiguous())   # W^T [Dp, H]
        dwf_t = ops.copy(dwf[li * H:(li + 1) * H].t(), torch.empty(Dp, H, device=dev, dtype=F32))
        dw_t, dgamma = ops.scale_rows_bwd(wt32, H, 0, dwf_t, H, 0, _f(lnm.weight), 1.0, Dp, 1, H)
        grads[lin.weight] = ops.copy(dw_t.t(), torch.empty(H, Dp, device=dev, dtype=F32))
        grads[lnm.weight] = dgamma
        if rec is None:
            # both biases add one constant per head to a whole softmax row: exact zeros (float64 autograd returns rounding noise)
            grads[lin.bias], grads[lnm.bias] = ops.zeros(H, device=dev, dtype=F32), ops.zeros(Dp, device=dev, dtype=F32)
        else:
            # (b' = W beta + b no longer drops out of the softmax: W receives db' beta^T through it as well)
            db = _copy(dbf[li * H:(li + 1) * H])
            grads[lin.bias] = db
            grads[lnm.bias] = ops.linear(db.view(1, H), wt32, None, out_dtype=F32, exact=True).view(Dp)
            dW = grads[lin.weight]
            ops.linear(db.view(H, 1), _f(lnm.bias).view(Dp, 1), None, out=dW, residual=dW, exact=True)
    return g, dpair, grads


class MsaUpdateWithPair(RecordingModule):
    """rf.py:598-610 (the reference hides these layers in a plain list; here they are registered).
    enable_backward() (switches every layer and each layer's FeedForward along): with grad mode on, forward(msa, pair) records,
    and loss.backward() fills the .grad of every parameter of the stack and of msa and pair where they require grad -- the one
    way a loss on the MSA track sends gradient into the pair track inside a block.  The backward (_backward) walks the layers in
    reverse; per layer: the feed-forward (FeedForward._backward through _pre_norm_residual_bwd, its dropouts replayed in train()
    mode), the attention-output dropout replayed, then with g the gradient of att . V
        d att[z,b,i,j] = sum_{n,c} g[b,n,i,h,c] v[b,n,j,h,c]          rf_gemm, K = N * dv in chunks of dv
        d v = att^T g                                                 rf_gemm on the transposed 16-bit map and g key-contiguous,
                                                                      both padded to map_ld(L) with zero columns
        dW_v, db_v = dv^T LN(msa), sum dv;   d LN(msa) = dv W_v       rf_conv_wgrad;  rf_gemm, exact fp32
        d msa += LayerNorm backward of msa2value[0]                   rf_layernorm_bwd
    LN(msa), the values and the maps are rebuilt from the saved tensors with the forward's own launches.  After the last layer
    all nl * H map gradients go through ONE rf_pair_softmax_bwd (dz [B,L,L,nl*H]), the logit dropout is replayed on dz,
    rf_conv_wgrad(dz, xs) with xs = rf_sym_layernorm(pair) gives the folded dW' and db', and rf_sym_layernorm_bwd gives d pair.
    The 16-bit copy of dz that rf_conv_wgrad reads (nl * H padded to a multiple of 8 with zero columns) is written by
    rf_pair_softmax_bwd itself in the bf16 mode without logit dropout; with logit dropout, and in the fp16 mode, it is written
    AFTER the replay and the fp16 scale, from the fp32 dz (the mask follows the element offset of the unpadded layout).
    The folded gradients are unfolded per layer: dW = dW' gamma, dgamma = sum_h dW' W, db = db', dbeta = W^T db'.  Without logit
    dropout pair2att.2.bias and pair2att.1.bias add one constant per head to a whole softmax row: their gradients are exact
    zeros; with it they are computed, and W receives the term db' beta^T through the folded bias b' = W beta + b as well.
    The fp16 mode's power-of-two gradient scale is applied per stage here (_rf_scales_own_grads), every backward contraction is
    pinned exact.  While recording, row_group is refused and d_msa, d_msa / n_heads and d_pair must be multiples of 8.
    TwoTrackBlock.run, ThreeTrackBlock.run3, FinalBlock.run3, RoseTTAFold.forward and the captured graph call run() without a
    tape: they never record here."""
    _rf_n_inputs = 2
    _rf_scales_own_grads = True

    def __init__(self, d_msa, d_pair, n_heads, n_encoder_layers=4, p_dropout=0.1):
        super().__init__()
        self.encoder_layers = nn.ModuleList([MsaUpdateWithPairLayer(d_msa, d_pair, n_heads, p_dropout)
                                             for _ in range(n_encoder_layers)])

    def run(self, msa, pair, row_group=None, tape=None):
        """msa fp32 [B,N,L,D] in place (replicated on every rank of row_group); pair: the whole tensor, or this rank's rows.
        tape: a dict that receives the front's and the layers' tapes (pair_to_att, MsaUpdateWithPairLayer.run; same kernels,
        same numbers)."""
        layers = list(self.encoder_layers)
        D = msa.shape[-1]
        _check_backward_call(self, tape, row_group, D, D // layers[0].n_heads, pair.shape[-1])
        if tape is not None:
            tape.update(front={}, layers=[{} for _ in layers])
        atts = pair_to_att(layers, pair, row_group, tape=tape["front"] if tape is not None else None)
        xn = None
        for i, (layer, att) in enumerate(zip(layers, atts)):
            nxt = layers[i + 1].msa2value[0] if i + 1 < len(layers) else None
            xn = layer.run(msa, att, xn=xn, next_ln=nxt, row_group=row_group,
                           tape=tape["layers"][i] if tape is not None else None)

    def _backward(self, tape, g, want_pair=True):
        """g: contiguous fp32 [B,N,L,D] gradient of the output (overwritten).  Returns (fp32 d msa [B,N,L,D], fp32 d pair
        [B,L,L,d_pair] or None, {param: grad}); the class docstring has the steps."""
        return _msa_update_with_pair_backward(list(self.encoder_layers), tape, g, want_pair)

    def _backward_children(self):
        return self.encoder_layers

    def _record(self, msa, pair, tape):
        msa = fresh_f32(msa)
        self.run(msa, pair.float().contiguous(), tape=tape)
        return msa

    _backward_from_autograd = MsaUpdateWithPairLayer._backward_from_autograd

    def forward(self, msa, pair):
        if _recording(self):
            return _RecordedFn.apply(self, msa, pair, *self.parameters())
        return self._record(msa, pair, None)


# ================================================================================================
# initial coordinates (graph transformer over the dense residue graph)
# ================================================================================================
class GraphTransformer(RecordingModule):
    """rf.py:613-664.  enable_backward(): with grad mode on, forward(node_feat, edge_feat, edge_mask) records, and
    loss.backward() fills the .grad of the five Linears and of node_feat and edge_feat where they require grad; edge_mask (None
    included) carries no gradient.  The backward rebuilds q, k, v, e from the saved inputs with the forward's projections and runs
    rf_graph_attention_bwd (include/rfmi.h); in train() mode it replays the forward's attention dropout.  A node with no edge
    attends uniformly whatever its logits: its query and every key and edge logit receive no gradient from that row, only the
    value path does -- the derivative of what the forward computes; the reference's autograd would differentiate logits that its
    own -1e9 rounds away, and is not followed.  Channel counts (d_node_in, d_edge, n_heads * d_node_out) must be multiples of 8
    while recording.  InitialCoordGenerationWithMsaAndPair calls run() with a tape only while it records itself;
    RoseTTAFold.forward reaches it without one and never records here."""
    _rf_n_inputs = 3   # node_feat, edge_feat, edge_mask (no gradient; may be None)

    def __init__(self, d_node_in, d_node_out, d_edge, n_heads, p_dropout=0.15):
        super().__init__()
        self.scale = d_node_out ** (-0.5)
        self.node_update = Linear(d_node_in, d_node_out * n_heads, bias=True)
        self.node_to_q = Linear(d_node_in, d_node_out * n_heads, bias=True)
        self.node_to_k = Linear(d_node_in, d_node_out * n_heads, bias=True)
        self.node_to_v = Linear(d_node_in, d_node_out * n_heads, bias=True)
        self.edge_emb = Linear(d_edge, d_node_out * n_heads, bias=False)
        self.n_heads, self.d_out = n_heads, d_node_out
        self.p_dropout = p_dropout   # rf.py:628,658: att_dropout on the attention probabilities

    def _projections(self, nt, edge_t):
        """q, k, v [B,L,H*d] and e [B,L,L,H*d] in T: the forward's four launches (the backward rebuilds them with the same ones)"""
        q = ops.linear(nt, self.wt("q", self.node_to_q), _f(self.node_to_q.bias))
        k = ops.linear(nt, self.wt("k", self.node_to_k), _f(self.node_to_k.bias))
        v = ops.linear(nt, self.wt("v", self.node_to_v), _f(self.node_to_v.bias))
        return q, k, v, ops.linear(edge_t, self.wt("e", self.edge_emb), None)

    def run(self, node, edge_t, mask=None, tape=None):
        """node fp32 [B,L,dn]; edge_t T [B,L,L,de] -> fp32 [B,L,H*d]; mask: None (the dense graph) or what edge_mask_u8 returns.
        tape: a dict that receives what _backward needs (the two inputs, the mask and the dropout record; same kernels, same
        numbers)."""
        B, Lr, _ = node.shape
        H, d = self.n_heads, self.d_out
        _check_backward_call(self, tape, None, node.shape[-1], edge_t.shape[-1], H * d)
        nt = ops.cast(node, T())
        q, k, v, e = self._projections(nt, edge_t)
        upd = torch.empty(B, Lr, H * d, device=node.device, dtype=F32)
        drop = None
        if self.training and self.p_dropout and self.p_dropout > 0:
            drop = (self.p_dropout, RT.train_seed, RT.train_offset)
            RT.train_offset += (B * H * Lr * Lr + 3) // 4
        ops.graph_attention(q, k, v, e, upd, B, Lr, H, d, self.scale, dropout=drop, mask=mask)
        if tape is not None:
            tape.update(node=node, edge_t=edge_t, mask=mask, drop=drop)
        return ops.linear(nt, self.wt("u", self.node_update), _f(self.node_update.bias), out_dtype=F32, residual=upd)

    def _backward(self, tape, g):
        """g: contiguous fp32 [B, L, H*d] gradient of the output (read only).  Returns (fp32 d node [B,L,dn], fp32 d edge
        [B,L,L,de], {param: grad}).  With q, k, v, e rebuilt from the saved inputs:
            dq, dk, dv, de = rf_graph_attention_bwd(q, k, v, e, g)             (the mask and the dropout record replayed)
            dW_x, db_x = dx^T node, sum dx   for x in q, k, v;   dW_u, db_u = g^T node, sum g;   dW_e = de^T edge     rf_conv_wgrad
            d node = dq W_q + dk W_k + dv W_v + g W_u,   d edge = de W_e                                               rf_gemm"""
        node, edge_t = tape["node"], tape["edge_t"]
        B, Lr, _ = node.shape
        H, d = self.n_heads, self.d_out
        nt = ops.cast(node, T())
        q, k, v, e = self._projections(nt, edge_t)
        dq, dk, dv, de, _, _ = ops.graph_attention_bwd(q, k, v, e, g, B, Lr, H, d, self.scale, dropout=tape["drop"], mask=tape["mask"])
        del q, k, v, e
        grads, dnode = {}, None
        for key, lin, dx in (("q", self.node_to_q, dq), ("k", self.node_to_k, dk), ("v", self.node_to_v, dv), ("u", self.node_update, g)):
            dx_t = ops.cast(dx, T())
            grads[lin.weight], grads[lin.bias] = ops.conv_wgrad(dx_t, nt, 1, bias=True)
            dnode = ops.linear(dx_t, self.wt_input_grad(key, lin), None, out=dnode, out_dtype=F32, residual=dnode, exact=True)
        grads[self.edge_emb.weight], _ = ops.conv_wgrad(de, edge_t, 1)
        dedge = ops.linear(de, self.wt_input_grad("e", self.edge_emb), None, out_dtype=F32, exact=True)
        return dnode, dedge, grads

    def _record(self, node_feat, edge_feat, edge_mask, tape):
        node = node_feat.float().contiguous()
        return self.run(node, ops.cast(edge_feat.float().contiguous(), T()), edge_mask_u8(edge_mask, node), tape=tape)

    def _backward_from_autograd(self, tape, gs, s, want):
        dnode, dedge, grads = self._backward(tape, _scaled_copy(gs[0], s))
        _unscale([dnode, dedge], s)
        return (dnode, dedge, None), grads

    def forward(self, node_feat, edge_feat, edge_mask):
        """edge_mask [B, L, L] (bool, uint8 or floating point; an edge exists where it equals 1) or None.  A node with at least
        one edge attends to its edges only.  A node with no edge attends uniformly (1/L) to every node: what the reference's
        (1 - mask) * -1e9 gives whenever every scaled logit lies in (-32, 32) (the float32 spacing at 1e9 is 64); outside that
        bound the reference's empty row is rounding noise and is not followed."""
        if _recording(self):
            return _RecordedFn.apply(self, node_feat, edge_feat, edge_mask, *self.parameters())
        return self._record(node_feat, edge_feat, edge_mask, None)


def edge_mask_u8(edge_mask, node):
    """The reference's edge_mask (rf.py:635) as the kernel's operand: uint8 [B, L, L] on node's device, 1 where the mask equals 1.
    No host read-back (the masked call stays capturable); any other shape raises ValueError before a launch."""
    if edge_mask is None:
        return None
    B, Lr, _ = node.shape
    if tuple(edge_mask.shape) != (B, Lr, Lr):
        raise ValueError(f"edge_mask must have shape [{B}, {Lr}, {Lr}] (b l l), got {tuple(edge_mask.shape)}")
    return (edge_mask.to(node.device) == 1).to(torch.uint8).contiguous()


class GraphTransformerBlock(RecordingModule):
    """rf.py:667-676.  enable_backward() (switches `attn` along): with grad mode on, forward(node_feat, edge_feat, edge_mask)
    records, and loss.backward() fills the .grad of to_out's Linear, the LayerNorm, every Linear of `attn`, and of node_feat and
    edge_feat where they require grad (see GraphTransformer for the mask, the node with no edge and the channel counts).
    InitialCoordGenerationWithMsaAndPair calls run() with a tape only while it records itself; RoseTTAFold.forward reaches it
    without one and never records here."""
    _rf_n_inputs = 3
    _rf_scales_own_grads = True   # the tail and the attention each at the fp16 mode's scale of their own gradient: _backward

    def __init__(self, d_node_in, d_node_out, d_edge, n_heads, p_dropout=0.15):
        super().__init__()
        self.attn = GraphTransformer(d_node_in, d_node_out, d_edge, n_heads, p_dropout)
        self.ln = LayerNorm(d_node_out * n_heads)
        self.to_out = nn.Sequential(Linear(d_node_out * n_heads, d_node_in), nn.ELU())

    def run(self, node, edge_t, mask=None, tape=None):
        """tape: a dict that receives what _backward needs (the attention's own tape, its fp32 output, the normalised rows and
        the block's output; same kernels, same numbers)."""
        sub = {} if tape is not None else None
        a = self.attn.run(node, edge_t, edge_mask_u8(mask, node), tape=sub)
        h = ln(self.ln, a)
        y = ops.linear(h, self.wt("o", self.to_out[0]), _f(self.to_out[0].bias), out_dtype=F32, act=L.ACT_ELU,
                       residual=node)
        if tape is not None:
            tape.update(attn=sub, a=a, h=h, node=node, y=y.detach())   # (an alias without autograd history: no reference cycle)
        return y

    def _backward(self, tape, g):
        """g: contiguous fp32 [B, L, dn] gradient of the output (read only).  Returns (fp32 d node, fp32 d edge, {param: grad}).
        y = node + ELU(h W_o + b_o), h = LayerNorm(attn):
            da = g * ELU'(y - node)                                rf_elu_bwd (the derivative from the activation's value)
            dW_o, db_o = da^T h, sum da;   dh = da W_o             rf_conv_wgrad, rf_gemm
            d attn, dgamma, dbeta = LayerNorm backward             rf_layernorm_bwd on the saved attention output
            d node, d edge = attn backward;   d node += g          the residual
        In the fp16 mode each of the two stages runs on a copy of its incoming gradient at a power-of-two scale of its own."""
        lin, lnm = self.to_out[0], self.ln
        s = _grad_scale([g])
        da = ops.elu_bwd(_scaled_copy(g, s), tape["y"], tape["node"], T())
        dw, db = ops.conv_wgrad(da, tape["h"], 1, bias=True)
        dh = ops.linear(da, self.wt_input_grad("o", lin), None, out_dtype=F32, exact=True)
        da_, dgamma, dbeta = ops.layernorm_bwd(tape["a"], dh, _f(lnm.weight), eps=lnm.eps)
        grads = {lin.weight: dw, lin.bias: db, lnm.weight: dgamma, lnm.bias: dbeta}
        _unscale([da_] + list(grads.values()), s)
        s = _grad_scale([da_])
        if s != 1.0:
            ops.axpby(da_, s, None, 0.0, da_)
        dnode, dedge, sub = self.attn._backward(tape["attn"], da_)
        _unscale([dnode, dedge] + list(sub.values()), s)
        grads.update(sub)
        ops.axpby(dnode, 1.0, g, 1.0, dnode)
        return dnode, dedge, grads

    def _backward_children(self):
        return (self.attn,)

    def _record(self, node_feat, edge_feat, edge_mask, tape):
        return self.run(node_feat.float().contiguous(), ops.cast(edge_feat.float().contiguous(), T()), edge_mask, tape=tape)

    def _backward_from_autograd(self, tape, gs, s, want):
        g = gs[0] if gs[0].dtype == F32 and gs[0].is_contiguous() else gs[0].float().contiguous()
        dnode, dedge, grads = self._backward(tape, g)
        return (dnode, dedge, None), grads

    def forward(self, node_feat, edge_feat, edge_mask):
        """edge_mask: as in GraphTransformer.forward."""
        if _recording(self):
            return _RecordedFn.apply(self, node_feat, edge_feat, edge_mask, *self.parameters())
        return self._record(node_feat, edge_feat, edge_mask, None)


def _node_input(mod, msa, seq_onehot, out_dtype=None, tape=None):
    """[sum_n w*LN(msa) | onehot] zero-padded to a multiple of 8 columns, T (rf.py:715-724, 789-798).
    tape: a dict that receives what _node_input_backward needs (msa, the type LayerNorm(msa) was kept in, and what
    weights_collapsed records; same kernels, same numbers)."""
    B, N, Lr, D = msa.shape
    # the fp32 (structure-track) form keeps LayerNorm(msa) in fp32 too: nothing upstream of the SE(3) stack is rounded
    m_dtype = F32 if (out_dtype == F32 and RT.struct_inputs_fp32) else None
    m = ln(mod.ln_msa, msa, out_dtype=m_dtype)
    w = mod.poswise_weight.weights_collapsed(msa, mod.ln_msa, m, tape=tape)
    if tape is not None:
        tape.update(msa=msa, m_dtype=m_dtype)
    Kp = pad8(D + 21)
    tmp = ops.zeros(B, Lr, Kp, device=msa.device, dtype=F32)
    ops.weighted_msa_sum(m, w, tmp, Kp)
    ops.copy(seq_onehot, tmp[..., D:D + 21])
    return ops.cast(tmp, out_dtype or T()), Kp


def _node_input_backward(mod, tape, ds):
    """Backward of _node_input (the front InitialCoordGenerationWithMsaAndPair and CoordUpdateWithMsaAndPair share) for ds =
    contiguous fp32 [B, L, D], the gradient of the first D columns of the node input (the one-hot columns carry none).  Returns
    (fp32 d msa, {param: grad}) over ln_msa and poswise_weight.  All of it runs in fp32, like the forward's q side.  With
    m = LN(msa) recomputed, q0 = to_q(LN(msa[:, 0])) and u = q0 W_k from the tape:
        du, dm = rf_poswise_bwd(u, m, ds)           the collapsed form with the weighted sum fused, the dropout record replayed
        dq0 = du W_k^T;   dW_k = sum_{b,l} q0 du^T;   db_k = 0 exactly (constant over n: it drops out of the softmax)
        dW_q, db_q = dq0^T row0, sum dq0;   dm[:, 0] += dq0 W_q
        d msa, dgamma, dbeta = LayerNorm backward of all rows at once        rf_layernorm_bwd"""
    msa = tape["msa"]
    B, N, Lr, D = msa.shape
    pw, lnm = mod.poswise_weight, mod.ln_msa
    lq, lk = pw.to_q[0], pw.to_k[0]
    m = ln(lnm, msa, out_dtype=tape["m_dtype"])
    du, dm = ops.poswise_bwd(tape["u"], D, m, D, 0, 0, D, B, N, Lr, 1, pw.scale, ds=ds, ds_ld=D, dk_dtype=F32,
                             dropout=tape["drop"])
    del m
    du, q0, row0 = du.view(B * Lr, D), tape["q0"].view(B * Lr, D), tape["row0"].view(B * Lr, D)
    dq0 = ops.linear(du, pw.cached("wk32", lambda: lk.weight.detach().float().contiguous()), None, out_dtype=F32, exact=True)
    grads = {lk.bias: ops.zeros(D, device=msa.device, dtype=F32)}
    grads[lk.weight], _ = ops.conv_wgrad(q0, du, 1)
    grads[lq.weight], grads[lq.bias] = ops.conv_wgrad(dq0, row0, 1, bias=True)
    wqt = pw.cached("wqt32", lambda: lq.weight.detach().float().t().contiguous())
    drow0 = ops.linear(dq0, wqt, None, out_dtype=F32, exact=True).view(B, Lr, D)
    for b in range(B):
        ops.axpby(dm[b, 0], 1.0, drow0[b], 1.0, dm[b, 0])
    dmsa, grads[lnm.weight], grads[lnm.bias] = ops.layernorm_bwd(msa, dm, _f(lnm.weight), eps=lnm.eps)
    return dmsa, grads


class InitialCoordGenerationWithMsaAndPair(RecordingModule):
    """rf.py:679-749.  enable_backward() (switches every block and its `attn` along): with grad mode on,
    forward(msa, pair, seq_onehot, aa_idx) records, and loss.backward() fills the .grad of every parameter of the module and of
    msa and pair where they require grad; seq_onehot and aa_idx carry no gradient.  The backward walks the forward in reverse:
    the output projection, the blocks (GraphTransformerBlock._backward, d edge summed over the blocks in fp32), the two ELU
    embeddings, the LayerNorm of pair, and the node input (_node_input_backward: rf_poswise_bwd in its fused collapsed form);
    in train() mode it replays the dropout on the softmax weights and the blocks' attention dropout.  poswise_weight.to_k.bias
    gets an exact zero.  d_msa, d_pair, d_node and d_edge must be multiples of 8 while recording.  RoseTTAFold.forward calls
    run() without a tape: it never records here."""
    _rf_n_inputs = 4   # msa, pair, seq_onehot (no gradient), aa_idx (no gradient)
    _rf_scales_own_grads = True   # every stage at the fp16 mode's scale of its own gradient: _backward

    def __init__(self, d_msa, d_pair, d_node=64, d_edge=64, n_heads=4, n_layers=4, p_dropout=0.1):
        super().__init__()
        self.ln_msa = LayerNorm(d_msa)
        self.ln_pair = LayerNorm(d_pair)
        self.poswise_weight = PositionWiseWeightFactor(d_msa, 1, p_dropout)
        self.node_embed = nn.Sequential(Linear(d_msa + 21, d_node), nn.ELU())
        self.edge_embed = nn.Sequential(Linear(d_pair + 1, d_edge), nn.ELU())
        self.blocks = nn.ModuleList([GraphTransformerBlock(d_node, d_node, d_edge, n_heads, p_dropout)
                                     for _ in range(n_layers)])
        self.to_out = Linear(d_node, 9)

    def run(self, msa, pair, seq_onehot, aa_idx, tape=None):
        """tape: a dict that receives what _backward needs (the node input's own tape, both embeddings' inputs and outputs, the
        blocks' tapes, pair; same kernels, same numbers)."""
        B, Lr, _, Dp = pair.shape
        _check_backward_call(self, tape, None, msa.shape[-1], Dp, self.node_embed[0].out_features, self.edge_embed[0].out_features)
        rec = tape is not None
        front = {} if rec else None
        Ke = pad8(Dp + 1)
        ein = ops.zeros(B, Lr, Lr, Ke, device=pair.device, dtype=T())
        nin, Kp = _node_input(self, msa, seq_onehot, tape=front)
        node = ops.linear(nin, self.wt("n", self.node_embed[0], kpad=Kp), _f(self.node_embed[0].bias), out_dtype=F32,
                          act=L.ACT_ELU)
        ln(self.ln_pair, pair, out=ein, out_ld=Ke)
        ops.seqsep_feature(aa_idx.contiguous(), ein, Ke, Dp)  # clamp(sign(d) log(|d|+1), 0, 5.5), rf.py:746-749
        edge = ops.linear(ein, self.wt("e", self.edge_embed[0], kpad=Ke), _f(self.edge_embed[0].bias), act=L.ACT_ELU)
        if rec:
            tape.update(front=front, nin=nin, node0=node, pair=pair, ein=ein, edge=edge, blocks=[])
        for blk in self.blocks:
            sub = {} if rec else None
            node = blk.run(node, edge, tape=sub)
            if rec:
                tape["blocks"].append(sub)
        if rec:
            tape["node"] = node.detach()
        xyz = ops.linear(ops.cast(node, T()), self.wt("o", self.to_out), _f(self.to_out.bias), out_dtype=F32)
        return xyz.view(B, Lr, 3, 3)

    def _backward(self, tape, g):
        """g: contiguous fp32 [B, L, 9] gradient of xyz (read only).  Returns (fp32 d msa, fp32 d pair, {param: grad}).
            d node = g W_o;   dW_o, db_o = g^T node, sum g        g zero-padded from 9 to 16 columns: the 16-bit weight gradient
                                                                  and rf_gemm take multiples of 8 (wt_input_grad's npad)
            d node, d edge += block backward, last block first     d edge summed over the blocks in fp32
            da_e = d edge * ELU'(edge)                             rf_elu_bwd on an fp32 copy of the operand-typed edge embedding,
                                                                  made here and freed after the call (the tape holds edge once)
            dW_e, db_e = da_e^T ein, sum da_e;   d pair = LayerNorm backward of (da_e W_e)[..., :d_pair]    (the sequence-separation
                                                                  column carries no gradient)
            da_n = d node * ELU'(node0);   dW_n, db_n = da_n^T nin, sum da_n;   ds = (da_n W_n)[..., :d_msa]
            d msa = _node_input_backward(ds)
        In the fp16 mode each stage runs on a copy of its incoming gradient at a power-of-two scale of its own."""
        B, Lr, _ = g.shape
        lo, ln_, le = self.to_out, self.node_embed[0], self.edge_embed[0]
        pair, nin, ein = tape["pair"], tape["nin"], tape["ein"]
        D, Dp = tape["front"]["msa"].shape[-1], pair.shape[-1]
        dev = g.device
        # ---- output projection
        s = _grad_scale([g])
        gp = ops.zeros(B * Lr, 16, device=dev, dtype=F32)
        ops.copy(_scaled_copy(g, s).view(B * Lr, 9), gp[:, :9])
        gp = ops.cast(gp, T())
        node_t = ops.cast(tape["node"], T()).view(B * Lr, -1)
        dw, db = ops.conv_wgrad(gp, node_t, 1, bias=True)
        grads = {lo.weight: dw[:9], lo.bias: db[:9]}
        dnode = ops.linear(gp, self.wt_input_grad("o", lo, npad=16), None, out_dtype=F32, exact=True).view(B, Lr, -1)
        _unscale([dnode] + list(grads.values()), s)
        # ---- blocks
        dedge = None
        for blk, sub in zip(reversed(self.blocks), reversed(tape["blocks"])):
            dnode, de, gr = blk._backward(sub, dnode)
            dedge = de if dedge is None else ops.axpby(dedge, 1.0, de, 1.0, dedge)
            grads.update(gr)
            del de
        if dedge is None:   # (no block: the edges reach nothing)
            dedge = ops.zeros(*tape["edge"].shape, device=dev, dtype=F32)
        # ---- edge embedding, LayerNorm(pair)
        s = _grad_scale([dedge])
        if s != 1.0:
            ops.axpby(dedge, s, None, 0.0, dedge)
        da = ops.elu_bwd(dedge, ops.cast(tape["edge"], F32), None, T())
        del dedge
        dw, db = ops.conv_wgrad(da, ein, 1, bias=True)
        we = self.cached("e_input_grad", lambda: le.weight.detach()[:, :Dp].t().to(T()).contiguous())
        dein = ops.linear(da, we, None, out_dtype=F32, exact=True)
        del da
        dpair, dgamma, dbeta = ops.layernorm_bwd(pair, dein, _f(self.ln_pair.weight), eps=self.ln_pair.eps)
        del dein
        gr = {le.weight: dw[:, :Dp + 1].contiguous(), le.bias: db, self.ln_pair.weight: dgamma, self.ln_pair.bias: dbeta}
        _unscale([dpair] + list(gr.values()), s)
        grads.update(gr)
        # ---- node embedding
        s = _grad_scale([dnode])
        da = ops.elu_bwd(_scaled_copy(dnode, s), tape["node0"], None, T())
        dw, db = ops.conv_wgrad(da, nin, 1, bias=True)
        wn = self.cached("n_input_grad", lambda: ln_.weight.detach()[:, :D].t().to(T()).contiguous())
        ds = ops.linear(da, wn, None, out_dtype=F32, exact=True)
        gr = {ln_.weight: dw[:, :D + 21].contiguous(), ln_.bias: db}
        _unscale([ds] + list(gr.values()), s)
        grads.update(gr)
        # ---- node input (fp32 throughout: no scale)
        dmsa, gr = _node_input_backward(self, tape["front"], ds)
        grads.update(gr)
        return dmsa, dpair, grads

    def _backward_children(self):
        return tuple(self.blocks)

    def _record(self, msa, pair, seq_onehot, aa_idx, tape):
        return self.run(msa.float().contiguous(), pair.float().contiguous(), seq_onehot.float(), aa_idx, tape=tape)

    def _backward_from_autograd(self, tape, gs, s, want):
        B, Lr = gs[0].shape[:2]
        dmsa, dpair, grads = self._backward(tape, gs[0].float().contiguous().view(B, Lr, 9))
        return (dmsa, dpair, None, None), grads

    def forward(self, msa, pair, seq_onehot, aa_idx):
        if _recording(self):
            return _RecordedFn.apply(self, msa, pair, seq_onehot, aa_idx, *self.parameters())
        return self._record(msa, pair, seq_onehot, aa_idx, None)


# ================================================================================================
# prediction head (ResNet over the pair map)
# ================================================================================================
class ResBlock2D(RecordingModule):
    """resnet.py:15-44."""

    def __init__(self, channel, kernel_size, dilation, p_dropout=0.15):
        super().__init__()
        self.dilation = dilation
        self.layer = Residual(nn.Sequential(
            nn.Conv2d(channel, channel, kernel_size, dilation=dilation, padding="same", bias=False),
            nn.InstanceNorm2d(channel, affine=True, eps=1e-6), nn.ELU(), nn.Dropout(p_dropout),
            nn.Conv2d(channel, channel, kernel_size, dilation=dilation, padding="same", bias=False),
            nn.InstanceNorm2d(channel, affine=True, eps=1e-6)))

    def _run_rows_b1(self, x_t, x_f, row_group, rows_global, next_halo):
        """Row block of ONE picture (a contiguous slab): the convolutions read pre-haloed buffers whose interiors the producers
        wrote directly -- only the halo rows move (shard.exchange_row_halos_inplace), no full-size copy."""
        from . import shard
        f, d = self.layer.fn, self.dilation
        _, h, W, Cc = x_t.shape
        kw = {"row_group": row_group, "rows_global": rows_global}
        xh = shard.haloed_parent(x_t, d)
        if xh is None:   # (the first block of a chain: its input was not produced into a haloed buffer)
            xh = shard.haloed_buffer(h, W, Cc, d, x_t.device, x_t.dtype)
            ops.axpby(x_t.contiguous(), 1.0, None, 0.0, shard.interior(xh, d))
        shard.exchange_row_halos_inplace(xh, d, row_group)
        y = conv3x3(self, "c1", f[0], xh, d)
        yh = shard.haloed_buffer(h, W, y.shape[-1], d, x_t.device, T())
        ops.instnorm(shard.interior(y, d), _f(f[1].weight), _f(f[1].bias), eps=f[1].eps, act=L.ACT_ELU, out=shard.interior(yh, d), **kw)
        shard.exchange_row_halos_inplace(yh, d, row_group)
        y = conv3x3(self, "c2", f[4], yh, d)
        nxt = shard.haloed_buffer(h, W, y.shape[-1], next_halo, x_t.device, T())
        o_f, o_t = ops.instnorm(shard.interior(y, d), _f(f[5].weight), _f(f[5].bias), eps=f[5].eps, residual=x_f, act=L.ACT_ELU,
                                out_dtype=F32, out2=shard.interior(nxt, next_halo), **kw)
        return o_t, o_f

    def run(self, x_t, x_f, row_group=None, rows_global=None, next_halo=0, tape=None):
        """x_t: T NHWC (conv input), x_f: fp32 copy (residual).  Returns (T, fp32) of elu(block(x)+x).
        row_group / rows_global: x holds a block of the picture's rows (shard.resblock_row_sharded): every convolution first
        fetches `dilation` rows from each neighbouring rank, the InstanceNorm sums are all-reduced.
        tape: a dict that receives what _backward needs (same kernels, same numbers): the convolutions' outputs (the norms'
        inputs), the InstanceNorm statistics, the ELU output before the dropout overwrites it, the dropout's (p, seed, offset),
        the output."""
        f = self.layer.fn
        kw = {} if row_group is None else {"row_group": row_group, "rows_global": rows_global}
        _check_backward_call(self, tape, row_group, x_t.shape[-1])
        rec = tape is not None
        if row_group is not None and x_t.shape[0] == 1:
            return self._run_rows_b1(x_t, x_f, row_group, rows_global, next_halo)

        def conv(key, c, x):
            if row_group is None:
                return conv3x3(self, key, c, x, self.dilation)
            from . import shard
            xh = shard.exchange_row_halos(x, self.dilation, row_group)
            return shard.drop_row_halos(conv3x3(self, key, c, xh, self.dilation), self.dilation)

        stats = [] if rec else None   # (every name below is rebound as before: the plain call frees what it always freed)
        y = conv("c1", f[0], x_t)
        if rec:
            tape.update(x_t=x_t, y1=y)
        y, _ = ops.instnorm(y, _f(f[1].weight), _f(f[1].bias), eps=f[1].eps, act=L.ACT_ELU, out_dtype=T(), stats_out=stats, **kw)
        p = _p(f[3]) if self.training else 0.0   # resnet.py:30
        if rec:
            tape["a1"] = _copy(y) if p > 0 else y
            tape["drop"] = _dropout_rec(y, p)
            tape["a1d"] = y
        else:
            dropout_(y, p)
        y = conv("c2", f[4], y)
        o_f, o_t = ops.instnorm(y, _f(f[5].weight), _f(f[5].bias), eps=f[5].eps, residual=x_f, act=L.ACT_ELU,
                                out_dtype=F32, out2_dtype=T(), stats_out=stats, **kw)
        if rec:
            tape.update(y2=y, s1=stats[0], s2=stats[1], o_f=o_f)
        return o_t, o_f

    def _backward(self, tape, g):
        """g: fp32 NHWC gradient of the block output (overwritten).  Returns (fp32 gradient of the block input, {param: grad})."""
        f, d = self.layer.fn, self.dilation
        # elu(IN2(conv2(.)) + x): g * elu' is both the residual branch's gradient (written back into g) and IN2's input
        dy2, dg5, db5 = ops.instnorm_bwd(g, tape["y2"], tape["s2"], _f(f[5].weight), eps=f[5].eps, act_out=tape["o_f"],
                                         dx_dtype=T(), ge_out=g)
        dw2, _ = ops.conv_wgrad(dy2, tape["a1d"], 9, d)
        da = conv3x3_input_grad(self, "c2", f[4], dy2, d)
        _replay_dropout(da, tape["drop"])
        dy1, dg1, db1 = ops.instnorm_bwd(da, tape["y1"], tape["s1"], _f(f[1].weight), eps=f[1].eps, act_out=tape["a1"],
                                         dx_dtype=T())
        dw1, _ = ops.conv_wgrad(dy1, tape["x_t"], 9, d)
        dx = conv3x3_input_grad(self, "c1", f[0], dy1, d, residual=g)
        return dx, {f[0].weight: _conv_weight_grad(dw1, f[0].weight), f[1].weight: dg1, f[1].bias: db1,
                    f[4].weight: _conv_weight_grad(dw2, f[4].weight), f[5].weight: dg5, f[5].bias: db5}

    def _record(self, x, tape):  # NCHW like the reference
        xf = x.float().permute(0, 2, 3, 1).contiguous()
        return self.run(ops.cast(xf, T()), xf, tape=tape)[1].permute(0, 3, 1, 2)

    def _backward_from_autograd(self, tape, gs, s, want_dx):
        dx, grads = self._backward(tape, _scaled_copy(gs[0].permute(0, 2, 3, 1), s))
        _unscale([dx], s)
        return dx.permute(0, 3, 1, 2), grads


class ResNet(RecordingModule):
    """resnet.py:47-83.  enable_backward(): this ResNet and its ResBlock2Ds."""

    def __init__(self, n_res_blocks, in_channels, intermediate_channels, out_channels, dilations=[1, 2, 4, 8],
                 p_dropout=0.15):
        super().__init__()
        layers = [nn.Conv2d(in_channels, intermediate_channels, 1, bias=False),
                  nn.InstanceNorm2d(intermediate_channels, affine=True, eps=1e-6), nn.ELU()]
        for b in range(n_res_blocks):
            layers.append(ResBlock2D(intermediate_channels, kernel_size=3, dilation=dilations[b % len(dilations)],
                                     p_dropout=p_dropout))
        layers.append(nn.Conv2d(intermediate_channels, out_channels, 1))
        self.layer = nn.Sequential(*layers)
        self.n_res_blocks = n_res_blocks

    def run(self, x_t, row_group=None, rows_global=None, tape=None):
        """x_t: T NHWC -> fp32 NHWC logits.  row_group / rows_global: x_t is a block of the picture's rows (see ResBlock2D.run).
        tape: a dict that receives what _backward needs (same kernels, same numbers) and the blocks' tapes."""
        l0, l1 = self.layer[0], self.layer[1]
        kw = {} if row_group is None else {"row_group": row_group, "rows_global": rows_global}
        _check_backward_call(self, tape, row_group, x_t.shape[-1], l0.weight.shape[0])
        rec = tape is not None
        s0 = [] if rec else None
        h = ops.linear(x_t, self.wt("in", l0), None)
        dil = [self.layer[3 + b].dilation for b in range(self.n_res_blocks)] + [0]
        if row_group is not None and h.shape[0] == 1:
            from . import shard
            first = shard.haloed_buffer(h.shape[1], h.shape[2], h.shape[3], dil[0], h.device, T())
            h_f, h_t = ops.instnorm(h, _f(l1.weight), _f(l1.bias), eps=l1.eps, act=L.ACT_ELU, out_dtype=F32,
                                    out2=shard.interior(first, dil[0]), **kw)
        else:
            h_f, h_t = ops.instnorm(h, _f(l1.weight), _f(l1.bias), eps=l1.eps, act=L.ACT_ELU, out_dtype=F32, out2_dtype=T(),
                                    stats_out=s0, **kw)
        if rec:
            tape.update(x_t=x_t, h0=h, s0=s0[0], h_f=h_f, blocks=[{} for _ in range(self.n_res_blocks)])
        for b in range(self.n_res_blocks):
            h_t, h_f = self.layer[3 + b].run(h_t, h_f, next_halo=dil[b + 1], tape=tape["blocks"][b] if rec else None, **kw)
        if rec:
            tape["h_last"] = h_t
        lo = self.layer[3 + self.n_res_blocks]
        return ops.linear(h_t, self.wt("out", lo), _f(lo.bias), out_dtype=F32)

    def _backward(self, tape, g, want_dx=True):
        """g: fp32 NHWC gradient of the logits (overwritten).  Returns (fp32 NHWC gradient of x_t or None, {param: grad})."""
        l0, l1 = self.layer[0], self.layer[1]
        lo = self.layer[3 + self.n_res_blocks]
        B, H, W, Co = g.shape
        C, Cin = lo.weight.shape[1], l0.weight.shape[1]
        co8 = pad8(Co)   # the 37 / 19 logit channels, zero-padded to 16-byte rows
        gp = ops.zeros(B, H, W, co8, device=g.device, dtype=T())
        ops.copy(g, gp[..., :Co])
        dwo, dbo = ops.conv_wgrad(gp, tape["h_last"], 1, bias=True)
        grads = {lo.weight: dwo[:Co].view(Co, C, 1, 1), lo.bias: dbo[:Co]}
        dh = ops.linear(gp, self.wt_input_grad("out", lo, co8), None, out_dtype=F32, exact=True)
        for b in reversed(range(self.n_res_blocks)):
            dh, gb = self.layer[3 + b]._backward(tape["blocks"][b], dh)
            grads.update(gb)
        dh0, dg, db = ops.instnorm_bwd(dh, tape["h0"], tape["s0"], _f(l1.weight), eps=l1.eps, act_out=tape["h_f"], dx_dtype=T())
        dwi, _ = ops.conv_wgrad(dh0, tape["x_t"], 1)
        grads.update({l0.weight: dwi.view(C, Cin, 1, 1), l1.weight: dg, l1.bias: db})
        dx = ops.linear(dh0, self.wt_input_grad("in", l0), None, out_dtype=F32, exact=True) if want_dx else None
        return dx, grads

    def _backward_children(self):
        return [m for m in self.layer if isinstance(m, ResBlock2D)]

    def _record(self, x, tape):  # NCHW in / NCHW out like the reference
        xf = x.float().permute(0, 2, 3, 1).contiguous()
        return self.run(ops.cast(xf, T()), tape=tape).permute(0, 3, 1, 2)

    def _backward_from_autograd(self, tape, gs, s, want_dx):
        dx, grads = self._backward(tape, _scaled_copy(gs[0].permute(0, 2, 3, 1), s), want_dx=want_dx)
        _unscale([dx], s)
        return (dx.permute(0, 3, 1, 2) if dx is not None else None), grads


_HEADS = ("theta", "phi", "dist", "omega")


class PredictionHead(RecordingModule):
    """rf.py:1130-1172.  enable_backward(): the head, its four ResNets and their ResBlock2Ds; forward() then returns logits that
    take part in autograd."""
    _rf_scales_own_grads = True   # each ResNet and the projection: _backward

    def __init__(self, in_channels, n_res_blocks, p_dropout):
        super().__init__()
        c = in_channels
        self.proj = nn.Sequential(LayerNorm(c), Linear(c, c), nn.Dropout(p_dropout), nn.Identity())
        self.dist_head = nn.Sequential(ResNet(n_res_blocks, c, c, 37, p_dropout=p_dropout), nn.Identity())
        self.omega_head = nn.Sequential(ResNet(n_res_blocks, c, c, 37, p_dropout=p_dropout), nn.Identity())
        self.theta_head = nn.Sequential(ResNet(n_res_blocks, c, c, 37, p_dropout=p_dropout), nn.Identity())
        self.phi_head = nn.Sequential(ResNet(n_res_blocks, c, c, 19, p_dropout=p_dropout), nn.Identity())

    def forward(self, pair):
        return dict(zip(_HEADS, super().forward(pair.float().contiguous())))

    def _record(self, pair, tape):
        out = self.run(pair, tape=tape)
        return tuple(out[k] for k in _HEADS)

    def _backward_children(self):
        return [getattr(self, name + "_head")[0] for name in _HEADS]

    def _backward_from_autograd(self, tape, gs, s, want_dx):
        return self._backward(tape, dict(zip(_HEADS, gs)), want_dpair=want_dx)

    def _backward(self, tape, gs, want_dpair=True):
        """gs: {name: gradient of that logit map}.  Returns (fp32 gradient of pair or None, {param: grad}): the unscaled
        gradients (each ResNet and the projection scale their own operands in the fp16 mode)."""
        grads, d = {}, {}
        for name in _HEADS:
            res = getattr(self, name + "_head")[0]
            s = _grad_scale([gs[name].float().contiguous()])
            d[name], gr = res._backward(tape[name], _scaled_copy(gs[name], s))
            _unscale([d[name]] + list(gr.values()), s)
            grads.update(gr)
        # x feeds theta / phi, xs = (x + x^T) / 2 feeds dist / omega (rf.py:1160)
        da = ops.axpby(d["dist"], 1.0, d["omega"], 1.0, d["dist"])
        dat = torch.empty_like(da)
        ops.copy(da.transpose(1, 2), dat)
        dx = ops.axpby(d["theta"], 1.0, d["phi"], 1.0, d["theta"])
        ops.axpby(dx, 1.0, da, 0.5, dx)
        ops.axpby(dx, 1.0, dat, 0.5, dx)
        # the 16-bit modes' centring of x (and of the projection's operand) is invariant for every consumer: no gradient term
        _replay_dropout(dx, tape["drop"])
        s = _grad_scale([dx])
        if s != 1.0:
            ops.axpby(dx, s, None, 0.0, dx)
        lin, lnm = self.proj[1], self.proj[0]
        dx_t = ops.cast(dx, T())
        dw, db = ops.conv_wgrad(dx_t, tape["op"], 1, bias=True)
        grads.update({lin.weight: dw, lin.bias: db})
        dpair = None
        if want_dpair or lnm.weight.requires_grad or lnm.bias.requires_grad:
            dt = ops.linear(dx_t, self.wt_input_grad("p", lin), None, out_dtype=F32, exact=True)
            dpair, dg, dbeta = ops.layernorm_bwd(tape["pair"], dt, _f(lnm.weight), eps=lnm.eps)
            grads.update({lnm.weight: dg, lnm.bias: dbeta})
        _unscale([dw, db, dpair, grads.get(lnm.weight), grads.get(lnm.bias)], s)
        return (dpair if want_dpair else None), grads

    def run(self, pair, row_group=None, tape=None):
        """pair fp32 [B, L, L, C] -> the four logit maps (fp32 NHWC).  row_group: `pair` is this rank's block of rows
        [B, h, L, C] (contiguous split shard.shard_range(L, world, rank)); the symmetrisation (rf.py:1160) fetches the
        transposed sub-blocks from the other ranks, the ResNets exchange halo rows and InstanceNorm sums; returns the same rows
        of the logit maps."""
        _, h, Lr, Cc = pair.shape
        _check_backward_call(self, tape, row_group, Cc, self.proj[1].weight.shape[0])
        kwc = {} if row_group is None else {"row_group": row_group, "rows_global": Lr}
        drop = None
        # Operand conditioning for the 16-bit modes (exact in exact arithmetic): every ResNet starts conv1x1 (no bias) ->
        # InstanceNorm (resnet.py:57-60), which is invariant to a per-channel constant of the conv's input, and the mean over
        # the picture of 0.5 (x + x^T) is the mean of x.  At random init that constant is ~19x the part that varies over the
        # picture (tools/precision_probe.py: the first InstanceNorm amplifies a white input error 19x), so x is rounded to 16
        # bits AFTER removing it -- and so is the projection's own operand LayerNorm(pair) (the other 6e-3 of the fp16 mode's
        # logits gap): W (t - mean t) is the projection minus ITS mean over the picture, bias and all.
        cond = RT.head_center and ops.is_h16(T()) and Cc % 4 == 0 and self.proj[1].weight.shape[0] % 4 == 0
        if cond and not self.training:
            t = ln(self.proj[0], pair, out_dtype=F32)
            op = ops.center_apply(t, ops.channel_mean(t, **kwc), out_dtype=T())
            x = ops.linear(op, self.wt("p", self.proj[1]), None, out_dtype=F32)
        else:
            op = ln(self.proj[0], pair)
            x = ops.linear(op, self.wt("p", self.proj[1]), _f(self.proj[1].bias), out_dtype=F32)
            if self.training:
                drop = _dropout_rec(x, _p(self.proj[2]))   # rf.py:1138 (the record goes on the tape, if there is one)
            if cond:
                ops.center_apply(x, ops.channel_mean(x, **kwc))
        if row_group is None:
            xt = torch.empty_like(x)
            ops.copy(x.transpose(1, 2), xt)
            kw = {}
        else:
            from . import shard
            xt = shard.transpose_row_sharded(x, row_group)
            kw = {"row_group": row_group, "rows_global": Lr}
        xs = ops.axpby(x, 0.5, xt, 0.5, torch.empty(x.shape, device=x.device, dtype=T()))
        x_t = ops.cast(x, T())
        if tape is not None:
            tape.update(pair=pair, op=op, drop=drop, **{name: {} for name in _HEADS})
        # x feeds theta / phi, xs = (x + x^T) / 2 feeds dist / omega (rf.py:1160)
        return {name: getattr(self, name + "_head")[0].run(xs if name in ("dist", "omega") else x_t,
                                                           tape=tape[name] if tape is not None else None, **kw)
                for name in _HEADS}
