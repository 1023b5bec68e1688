"""Thin Python wrappers over the C ABI of librfmi.so (include/rfmi.h).

PyTorch is used here for device memory (tensors), the current HIP stream and dtype tags only;
every arithmetic step is a kernel of librfmi.so reached through ctypes with raw device pointers.

Device rule: every operand of a call lives on ONE device and that device is the calling thread's current device
(kernels are enqueued on its current stream); anything else raises RfmiError instead of launching on the wrong GPU.
`RoseTTAFold.forward` enters `torch.cuda.device(input.device)` itself, so the model can live on any GPU.
"""
import ctypes as C

import torch

from . import _lib as L
from ._lib import lib, check, GemmDesc, I64x4, I64x3

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
_H16_CODE = {torch.bfloat16: L.RF_BF16, torch.float16: L.RF_F16}
_H16_TORCH = {L.RF_BF16: torch.bfloat16, L.RF_F16: torch.float16}


def is_h16(dtype):
    """A 16-bit MFMA operand type (bfloat16: librfmi.so, float16: librfmi_f16.so)."""
    return dtype in _H16_CODE


def h16():
    """torch dtype of the 16-bit operand type of the library that is active now (model.set_compute_dtype)."""
    return _H16_TORCH[L.active_h16()]


def dcode(dtype):
    if dtype == torch.float32:
        return L.RF_F32
    code = _H16_CODE.get(dtype)
    if code is None:
        raise TypeError(f"unsupported dtype {dtype}")
    if code != L.active_h16():  # (the library would reject the code too: this names the cause)
        raise L.RfmiError(f"{dtype} tensor passed while the active library computes in {h16()} "
                          "(set_compute_dtype selects the library)")
    return code


# set by model.set_compute_dtype / model.set_float32_matmul_precision: True in float32 mode with the "high" precision
_SPLIT_F32 = False


def set_split_f32(on):
    global _SPLIT_F32
    _SPLIT_F32 = bool(on)


def gemm_code(dtype, exact=False):
    """rf_gemm_desc.ab_dtype of an A/B dtype: float32 operands take the split-bf16 kernel (RF_F32X3) while the "high" float32
    matmul precision is in effect (model.set_float32_matmul_precision), unless the call pins the exact fp32 kernel."""
    code = dcode(dtype)
    return L.RF_F32X3 if code == L.RF_F32 and _SPLIT_F32 and not exact else code


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t, off_elems=0):
    if t is None:
        return None
    if t.dtype in _H16_CODE and _H16_CODE[t.dtype] != L.active_h16():
        # entry points without a dtype argument read 16-bit memory as the active library's type: never hand them the other one
        raise L.RfmiError(f"{t.dtype} tensor passed while the active library computes in {h16()}")
    return C.c_void_p(t.data_ptr() + off_elems * t.element_size())


def _i4(v):
    return C.byref(I64x4(*[int(x) for x in v]))


def _need_cuda(*ts):
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise L.RfmiError("librfmi ops need device tensors (there is no CPU fallback)")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise L.RfmiError(f"operands on different devices: {dev} and {t.device}")
    if dev is not None and dev.index != torch.cuda.current_device():
        raise L.RfmiError(f"operands live on {dev} but the current device is cuda:{torch.cuda.current_device()} "
                          "(wrap the call in torch.cuda.device(...))")


# --------------------------------------------------------------------------------------------- GEMM
def gemm(A, B, Cout, M, N, K, *, batch=(1, 1, 1), a_off=0, b_off=0, c_off=0,
         a_bs=(0, 0, 0), a_row=(0, 0, None), a_ko=0,
         b_bs=(0, 0, 0), b_row=(0, 0, None), b_ko=0, kc=0,
         c_bs=(0, 0, 0), c_row=(0, 0, None), c_col=(0, 0),
         bias=None, bias_mode=None, act=L.ACT_NONE, act_nvalid=0, act_eps=0.0, alpha=1.0,
         residual=None, res_off=None, conv=None, tile_cfg=0, ln=None, block_ln=None, rs=None, exact=False):
    """C = epilogue(alpha * A @ B^T) with the strided/batched/chunked addressing of rf_gemm_desc.
    *_row = (rc, ro, ri): offset(m) = (m // rc)*ro + (m % rc)*ri, rc=0 -> m*ri.  ri=None -> K (A,B) / N (C).
    c_col = (cc, co).  Offsets are in elements.  conv = (n, h, w, c, dilation) selects implicit 3x3 im2col.
    exact=True keeps fp32 operands on the exact fp32 kernel whatever the float32 matmul precision (gemm_code)."""
    _need_cuda(A, B, Cout, bias, residual)
    if A.dtype != B.dtype:
        raise TypeError("A and B dtypes differ")
    d = GemmDesc()
    d.M, d.N, d.K = int(M), int(N), int(K)
    d.nb0, d.nb1, d.nb2 = [int(x) for x in batch]
    d.ab_dtype, d.c_dtype = gemm_code(A.dtype, exact), dcode(Cout.dtype)
    d.kc = int(kc)
    d.a_rc, d.a_ro, d.a_ri = int(a_row[0]), int(a_row[1]), int(K if a_row[2] is None else a_row[2])
    d.b_rc, d.b_ro, d.b_ri = int(b_row[0]), int(b_row[1]), int(K if b_row[2] is None else b_row[2])
    d.c_rc, d.c_ro, d.c_ri = int(c_row[0]), int(c_row[1]), int(N if c_row[2] is None else c_row[2])
    d.c_cc, d.c_co = int(c_col[0]), int(c_col[1])
    for i in range(3):
        d.a_bs[i], d.b_bs[i], d.c_bs[i] = int(a_bs[i]), int(b_bs[i]), int(c_bs[i])
    d.a_ko, d.b_ko = int(a_ko), int(b_ko)
    if conv is not None:
        d.a_mode = L.AMODE_CONV3X3
        d.conv_n, d.conv_h, d.conv_w, d.conv_c, d.conv_dil = [int(x) for x in conv]
    if bias is not None:
        if bias.dtype != F32:
            raise TypeError("bias must be fp32")
        d.bias_mode = L.BIAS_COL if bias_mode is None else bias_mode
        d.bias = bias.data_ptr()
    d.act, d.act_nvalid, d.act_eps, d.alpha = int(act), int(act_nvalid), float(act_eps), float(alpha)
    d.tile_cfg = int(tile_cfg)
    d.A = A.data_ptr() + a_off * A.element_size()
    d.B = B.data_ptr() + b_off * B.element_size()
    d.C = Cout.data_ptr() + c_off * Cout.element_size()
    if residual is not None:
        if residual.dtype != F32:
            raise TypeError("residual must be fp32")
        d.residual = residual.data_ptr() + (c_off if res_off is None else res_off) * 4
    if block_ln is not None:  # (gamma[1024], beta[1024], eps) with act=ACT_BLOCK_LN32: LayerNorm over 32x32 output blocks
        g, b, eps = block_ln
        _need_cuda(g, b)
        d.ln_gamma, d.ln_beta, d.ln_eps = g.data_ptr(), b.data_ptr(), float(eps)
    if rs is not None:  # (scale fp32, bstride, rpb, cg, ncols, alpha): row-group scale of the leading columns (rf_gemm_desc.rs)
        t_, bstride, rpb, cg, ncols, alpha_ = rs
        _need_cuda(t_)
        if t_.dtype != F32:
            raise TypeError("rs must be fp32")
        d.rs, d.rs_bstride, d.rs_rpb, d.rs_cg, d.rs_ncols, d.rs_alpha = t_.data_ptr(), int(bstride), int(rpb), int(cg), int(ncols), float(alpha_)
    if ln is not None:  # (out bf16 [M,N], gamma, beta, eps): fused LayerNorm of the result rows
        ln_out, g, b, eps = ln
        _need_cuda(ln_out, g, b)
        d.ln_out, d.ln_gamma, d.ln_beta, d.ln_eps = ln_out.data_ptr(), g.data_ptr(), b.data_ptr(), float(eps)
    check(lib.rf_gemm(C.byref(d), stream()), "rf_gemm")
    return Cout


_NO_WREG = bool(int(__import__("os").environ.get("RF_NO_WREG_GEMM", "0") or "0"))


def gemm_takes_row_scale(M, N, K):
    """The row-group scale (`rs=` of gemm) lives in the epilogue of the register-resident-weights kernel only
    (csrc/gemm_wreg.hip: rf_gemm_wreg_try); every other kernel answers RF_EINVAL to it.  True when a plain 16-bit
    projection of this shape goes to that kernel, i.e. when a caller may fold its per-row factor into the GEMM."""
    return (not _NO_WREG) and K in (288, 384) and M % 64 == 0 and M >= 16384 and N % 128 == 0 and N >= 256  # (+ a split-C output)


def linear(x, w, bias=None, *, out=None, out_dtype=None, act=L.ACT_NONE, residual=None, alpha=1.0, tile_cfg=0, ln=None,
           exact=False):
    """out[..., N] = act(x[..., K] @ w[N, K]^T + bias) (+ residual).  x contiguous, w [N, Kw>=K] contiguous."""
    K = x.shape[-1]
    Mrows = x.numel() // K
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"linear: K mismatch {w.shape} vs {x.shape}")
    if out is None:
        out = torch.empty(*x.shape[:-1], N, device=x.device, dtype=out_dtype or x.dtype)
    gemm(x, w, out, Mrows, N, K, bias=bias, act=act, residual=residual, alpha=alpha, tile_cfg=tile_cfg, ln=ln, exact=exact)
    return out


# --------------------------------------------------------------------------------------------- norms
def layernorm(x, gamma, beta, *, eps=1e-5, out=None, out_dtype=None, out_ld=None, out_off=0, rows=None, D=None,
              x_ld=None, groups=1, act=L.ACT_NONE):
    D = x.shape[-1] if D is None else D
    rows = x.numel() // D if rows is None else rows
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=out_dtype or x.dtype)
    _need_cuda(x, out, gamma, beta)
    check(lib.rf_layernorm(ptr(x), dcode(x.dtype), D if x_ld is None else x_ld, ptr(out, out_off), dcode(out.dtype),
                           D if out_ld is None else out_ld, rows, D, ptr(gamma), ptr(beta), eps, groups, act,
                           stream()), "rf_layernorm")
    return out


def sym_layernorm(pair, out_dtype, eps=1e-5):
    B, L_, _, D = pair.shape
    out = torch.empty(pair.shape, device=pair.device, dtype=out_dtype)
    _need_cuda(pair)
    check(lib.rf_sym_layernorm(ptr(pair), ptr(out), dcode(out_dtype), B, L_, D, eps, stream()), "rf_sym_layernorm")
    return out


def softmax(x, x_off, x_rs, x_cs, y, y_off, y_rs, rows, cols, scale=1.0):
    _need_cuda(x, y)
    check(lib.rf_softmax(ptr(x, x_off), x_rs, x_cs, ptr(y, y_off), dcode(y.dtype), y_rs, rows, cols, scale, stream()),
          "rf_softmax")


def softmax_batched(x, x_bs, x_rs, x_cs, y, y_bs, y_rs, rows, cols, nbatch, scale=1.0):
    _need_cuda(x, y)
    check(lib.rf_softmax_batched(ptr(x), x_bs, x_rs, x_cs, ptr(y), dcode(y.dtype), y_bs, y_rs, rows, cols, scale, nbatch,
                                 stream()), "rf_softmax_batched")


def tied_logits_softmax(q, k, b_stride, n_stride, l_stride, att, att_sym, B, H, N, L_, d_head):
    """att[b,h,i,:] = softmax_j(sum_{n,d} q k) in one launch (csrc/tied.hip); q, k: bf16 views into the projection output."""
    _need_cuda(q, k, att, att_sym)
    check(lib.rf_tied_logits_softmax(ptr(q), ptr(k), b_stride, n_stride, l_stride, ptr(att), ptr(att_sym),
                                     att_sym.shape[-1] if att_sym is not None else 0, B, H, N, L_, d_head, stream()),
          "rf_tied_logits_softmax")
    return att


def _hstrides(t):
    """(b, n, h, l) element strides of a [B, N, H, L, 32]-indexed view (head slice contiguous)."""
    if t.dim() != 5 or t.stride(4) != 1 or t.shape[4] != 32:
        raise ValueError("expected a [B, N, H, L, 32] view with a contiguous head dimension")
    return I64x4(t.stride(0), t.stride(1), t.stride(2), t.stride(3))


TIED_TILES = (64, 128, 192, 256)  # chain lengths that fill a tile of the fused tied-attention kernels


def tied_ld(L_):
    """Leading dimension of a 16-bit attention map (and of key-contiguous values) of a chain of L residues: L rounded up to a
    multiple of 8, so that every row is 16-byte aligned and the contraction over it is a legal K of the 16-bit GEMM."""
    return (L_ + 7) // 8 * 8


def tied_lds_fits(L_, w_rows):
    """The one-pass logits kernel's LDS at a chain of 1 <= L <= 256 residues fits the 160 KB of a workgroup (csrc/tied.hip:
    launch_tied): a ring of 6 (tile 256) or 8 stages of a 64-query and a key tile, 1 KB, and 256 bytes per MSA row of a
    position-weight tile of w_rows rows."""
    tile = (L_ + 63) // 64 * 64
    return (6 if tile >= 256 else 8) * (4096 + tile * 64) + 1024 + w_rows * 256 <= 160 * 1024


def tied_fused_applies(L_, N, dtype, dh=32, w=True):
    """Python mirror of what rf_tied_attention_ld accepts (the one-pass logits + softmax kernel, then attention . V): 16-bit
    operands, d_head 32, 1 <= L <= 256, and a ring + position-weight tile that fit the LDS (w: the weights are applied in the
    kernel, which stages them four MSA rows per DMA instruction)."""
    if not (is_h16(dtype) and dh == 32 and 1 <= L_ <= 256 and N >= 1):
        return False
    if w and N % 4:
        return False
    return tied_lds_fits(L_, N if w else 0)


def _att_ld(att, L_):
    """att: [B, H, L, att_ld] contiguous with att_ld >= L (columns past L: the zero pad the kernels write)."""
    if att.dim() != 4 or not att.is_contiguous() or att.shape[2] != L_ or att.shape[3] < L_:
        raise ValueError("att must be a contiguous [B, H, L, att_ld] tensor with att_ld >= L")
    return att.shape[3]


def _w_strides(w, B, H, N, L_):
    if w is None:
        return I64x3(0, 0, 0)
    if w.dim() != 4 or w.stride(3) != 1 or tuple(w.shape[:3]) != (B, H, N) or w.shape[3] < L_:
        raise ValueError("w must be [B, H, N, >= L] with contiguous L")
    return I64x3(w.stride(0), w.stride(1), w.stride(2))


def _qk_sym(q, k, att_sym):
    """(strides shared by the head-major q and k views, row pitch of att_sym or 0) as the logits entry points take them"""
    if q.stride() != k.stride():
        raise ValueError("q and k must share their strides")
    return C.byref(_hstrides(q)), att_sym.shape[-1] if att_sym is not None else 0


def tied_attention(q, k, v, out, att, w=None, qscale=1.0, att_sym=None, partial_ws=None):
    """Tied MSA-row attention core (csrc/tied.hip).  q, k, v, out: bf16 views indexed [B, N, H, L, 32] (any strides with
    a contiguous head slice); att: bf16 [B, H, L, att_ld] (workspace + result; att_ld = L, or any multiple of 8 >= L: the
    kernels write zeros past column L); w: fp32 [B, H, N, L] position weights folded into the logits kernel (None: q already
    carries them; rows padded to a multiple of 4 floats when L % 4 != 0); att_sym: fp32 [B, L, L, H] or None.  partial_ws: fp32
    workspace for the contraction-split logits (L == 256); allocated here when None, pass False to force the one-pass kernel.
    A chain that fills a tile (L in TIED_TILES, dense att) goes to rf_tied_attention, every other to rf_tied_attention_ld."""
    B, N, H, L_, dh = q.shape
    att_ld = _att_ld(att, L_)
    if partial_ws is None and L_ == 256 and att_ld == L_ and N % 2 == 0:
        partial_ws = torch.empty((4 if N > 128 else 2) * B * H * L_ * L_, device=q.device, dtype=F32)
    if partial_ws is False:
        partial_ws = None
    _need_cuda(q, k, v, out, att, w, att_sym, partial_ws)
    qks, sym_ld = _qk_sym(q, k, att_sym)
    ws = _w_strides(w, B, H, N, L_)
    ws_elems = partial_ws.numel() if partial_ws is not None else 0
    if not (L_ in TIED_TILES and att_ld == L_):
        check(lib.rf_tied_attention_ld(ptr(q), ptr(k), ptr(v), qks, C.byref(_hstrides(v)), ptr(w), C.byref(ws), float(qscale),
                                       ptr(att), att_ld, ptr(att_sym), sym_ld, ptr(out), C.byref(_hstrides(out)), B, H, N, L_, dh,
                                       ptr(partial_ws), ws_elems, stream()), "rf_tied_attention_ld")
        return out
    check(lib.rf_tied_attention(ptr(q), ptr(k), ptr(v), qks, C.byref(_hstrides(v)), ptr(w), C.byref(ws), float(qscale), ptr(att),
                                ptr(att_sym), sym_ld, ptr(out), C.byref(_hstrides(out)), B, H, N, L_, dh, ptr(partial_ws),
                                ws_elems, stream()), "rf_tied_attention")
    return out


COUNTERS = {"tied_logits_long": 0}  # launches of paths a test wants to see taken


def tied_logits_ld(q, k, att, w=None, qscale=1.0, att_sym=None):
    """rf_tied_logits_ld on head-major q / k views [B, N, H, L, 32], one-pass kernel: att 16-bit [B, H, L, att_ld] (see
    tied_attention), any 1 <= L <= 256."""
    B, N, H, L_, dh = q.shape
    att_ld = _att_ld(att, L_)
    _need_cuda(q, k, att, w, att_sym)
    qks, sym_ld = _qk_sym(q, k, att_sym)
    check(lib.rf_tied_logits_ld(ptr(q), ptr(k), qks, ptr(w), C.byref(_w_strides(w, B, H, N, L_)), float(qscale), ptr(att), att_ld,
                                ptr(att_sym), sym_ld, B, H, N, L_, dh, None, 0, stream()), "rf_tied_logits_ld")
    return att


def tied_av_ld(att, v, out):
    """rf_tied_av_ld: att 16-bit [B, H, L, att_ld] with zeros past column L, v / out views [B, N, H, L, 32], 1 <= L <= 256."""
    B, N, H, L_, dh = v.shape
    att_ld = _att_ld(att, L_)
    _need_cuda(att, v, out)
    check(lib.rf_tied_av_ld(ptr(att), att_ld, ptr(v), C.byref(_hstrides(v)), ptr(out), C.byref(_hstrides(out)), B, H, N, L_, dh,
                            stream()), "rf_tied_av_ld")
    return out


def tied_logits(q, k, att, att_sym=None, qscale=1.0):
    """Logits + softmax of the tied attention on head-major q / k views [B, N, H, L, 32] (position weights already folded
    into q): att 16-bit [B, H, L, L], att_sym fp32 [B, L, L, H] or None.  L in {512, 768, 1024} (BASELINE.json configs[3]):
    contraction-split kernel over 128-query x 256-key tiles with an fp32 workspace (csrc/tied.hip: rf_tied_logits)."""
    B, N, H, L_, dh = q.shape
    nsplit = 1
    while N // nsplit > 64 and N % (2 * nsplit) == 0:
        nsplit *= 2
    ws = torch.empty(max(nsplit, 2 if L_ == 256 else 1) * B * H * L_ * L_, device=q.device, dtype=F32)
    _need_cuda(q, k, att, att_sym, ws)
    qks, sym_ld = _qk_sym(q, k, att_sym)
    check(lib.rf_tied_logits(ptr(q), ptr(k), qks, None, C.byref(I64x3(0, 0, 0)), float(qscale), ptr(att), ptr(att_sym), sym_ld,
                             B, H, N, L_, dh, ptr(ws), ws.numel(), stream()), "rf_tied_logits")
    if L_ > 256:
        COUNTERS["tied_logits_long"] += 1
    return att


def _tied_long_splits(N, B=1, H=1, L_=512):
    """MSA-row ranges of the contraction-split logits kernel above L = 256, from the library's workspace size; 0: N is outside it"""
    return lib.rf_tied_logits_long_ws_elems(B, H, N, L_) // (B * H * L_ * 256 * ((L_ + 255) // 256))


def tied_long_applies(L_, N, dtype, dh=32):
    """What rf_tied_logits_long accepts: 16-bit operands, d_head 32, 257 <= L <= 1024 and an MSA depth its split rule takes (N
    even, ranges of 4 .. 64 and an even number of MSA rows), asked of the library's host-only rf_tied_logits_long_ws_elems."""
    return bool(is_h16(dtype) and dh == 32 and 257 <= L_ <= 1024 and _tied_long_splits(N, L_=L_))


def tied_logits_long(q, k, att, att_sym=None, qscale=1.0):
    """tied_logits at any chain length 257 <= L <= 1024 (rf_tied_logits_long: the tail instantiations of the contraction-split
    kernel): att 16-bit [B, H, L, att_ld], att_ld >= L a multiple of 8, zeros written past column L."""
    B, N, H, L_, dh = q.shape
    att_ld = _att_ld(att, L_)
    # (a refused shape gets 4 floats and the library's answer)
    ws = torch.empty(max(lib.rf_tied_logits_long_ws_elems(B, H, N, L_), 4), device=q.device, dtype=F32)
    _need_cuda(q, k, att, att_sym, ws)
    qks, sym_ld = _qk_sym(q, k, att_sym)
    check(lib.rf_tied_logits_long(ptr(q), ptr(k), qks, float(qscale), ptr(att), att_ld, ptr(att_sym), sym_ld, B, H, N, L_, dh,
                                  ptr(ws), ws.numel(), stream()), "rf_tied_logits_long")
    COUNTERS["tied_logits_long"] += 1
    return att


def tied_row_attention(q, k, v):
    """Functional form for the dispatcher op: q, k, v h16 [B, N, L, H, 32] -> (out [B, N, L, H*32], att_sym [B, L, L, H]).
    L in TIED_TILES, or any 1 <= L <= 256 (the attention map then has the leading dimension tied_ld(L): rf_tied_attention_ld)."""
    B, N, L_, H, dh = q.shape
    out = torch.empty(B, N, L_, H * dh, device=q.device, dtype=q.dtype)
    att = torch.empty(B, H, L_, tied_ld(L_), device=q.device, dtype=q.dtype)
    sym = torch.empty(B, L_, L_, H, device=q.device, dtype=F32)
    hm = lambda t: t.permute(0, 1, 3, 2, 4)  # noqa: E731  [B, N, H, L, 32] view
    tied_attention(hm(q.contiguous()), hm(k.contiguous()), hm(v.contiguous()), hm(out.view(B, N, L_, H, dh)), att, att_sym=sym)
    return out, sym


def outer_fused(xt, yt, wprime, s, c, out, eps, ln2=None):
    """Fused OuterProductMean core (csrc/outer.hip): xt 16-bit [B, Li, 32, N] (rows of the picture), yt 16-bit [B, Lj, 32, N] (its
    columns), any Li, Lj >= 1, N = 64 or 128 (outer_depth); wprime chunk-major [16, Dout, 64] from outer_fold; out fp32 [B,Li,Lj,Dout].
    ln2 = (gamma, beta, eps, y, y_ld): also apply LayerNorm over Dout and write 16-bit y[(b,i,j) * y_ld + o] instead of `out`."""
    B, Li, P, N = xt.shape
    Lj = yt.shape[1]
    if yt.dim() != 4 or (yt.shape[0], yt.shape[2], yt.shape[3]) != (B, P, N) or not (xt.is_contiguous() and yt.is_contiguous()):
        raise ValueError(f"outer_fused: contiguous operands [B, Li, P, N] and [B, Lj, P, N] expected, got {tuple(xt.shape)} and "
                         f"{tuple(yt.shape)}")
    if out is not None and (out.dtype != F32 or tuple(out.shape) != (B, Li, Lj, wprime.shape[1]) or not out.is_contiguous()):
        raise ValueError(f"outer_fused: out must be contiguous fp32 {(B, Li, Lj, wprime.shape[1])}")
    _need_cuda(xt, yt, wprime, s, c, out)
    g2 = b2 = y = None
    eps2, y_ld = 0.0, 0
    if ln2 is not None:
        g2, b2, eps2, y, y_ld = ln2
        _need_cuda(g2, b2, y)
    if wprime.dim() != 3 or wprime.shape[0] != 16 or wprime.shape[2] != 64:
        raise ValueError("outer_fused: wprime must come from outer_fold (chunk-major [16, Dout, 64])")
    check(lib.rf_outer_product_ln_linear_rect(ptr(xt), ptr(yt), ptr(wprime), ptr(s), ptr(c), ptr(out), B, Li, Lj, N, P,
                                              wprime.shape[1], float(eps), ptr(g2), ptr(b2), float(eps2), ptr(y), int(y_ld),
                                              stream()),
          "rf_outer_product_ln_linear_rect")
    return y if ln2 is not None else out


def outer_fold(w, gamma, beta, bias, dtype=None):
    """(W * gamma in the 16-bit type in kernel layout, its fp32 row sums, W beta + bias): the LayerNorm(1024) affine folded into
    Linear(1024 -> Dout).  Layout: chunk-major [16 chunks = (ug, vg)][Dout][64 = (uu, vv)] with feature k = (8 ug + uu) * 32 +
    8 vg + vv: the 64 features a chunk of csrc/outer.hip contracts over are one 128-byte line per output column."""
    wp = (w.float() * gamma.float()[None, :]).to(dtype or h16()).contiguous()
    s = wp.float().sum(1).contiguous()
    Dout = wp.shape[0]
    c = (w.float() @ beta.float() + bias.float()).contiguous()
    wpc = wp.view(Dout, 4, 8, 4, 8).permute(1, 3, 0, 2, 4).contiguous().view(16, Dout, 64)
    return wpc, s, c


def outer_depth(N):
    """MSA depth the fused kernel (csrc/outer.hip) runs a depth-N outer product at: 64 or 128, zero-padded (zeros add nothing
    to the sum over n); None for N > 128 (eight K steps of operands do not fit the LDS: the general route)."""
    return 64 if N <= 64 else 128 if N <= 128 else None


def outer_pad_depth(t, Np):
    """t [B, L, P, n] -> contiguous [B, L, P, Np], zero-padded along the MSA depth (t itself when n == Np already)."""
    B, L_, P, n = t.shape
    if n == Np and t.is_contiguous():
        return t
    out = zeros(B, L_, P, Np, device=t.device, dtype=t.dtype)
    copy(t, out[..., :n])
    return out


def outer_operands(x, y, dtype, multiple=8):
    """Transposed operands of the outer product: x, y [B, N, L, P] -> (xt, yt `dtype` [B, L, P, Np], Np) with the MSA depth
    contiguous and zero-padded to Np = a multiple of `multiple`: 8 (the contraction granule of the GEMM route) or the fused
    kernel's depth outer_depth(N)."""
    B, N, L_, P = x.shape
    Np = (N + multiple - 1) // multiple * multiple
    mk = zeros if Np != N else torch.empty  # only the K padding needs zeros
    xt = mk(B, L_, P, Np, device=x.device, dtype=dtype)
    yt = mk(B, L_, P, Np, device=x.device, dtype=dtype)
    for src, dst in ((x, xt), (y, yt)):
        copy(src.permute(0, 2, 3, 1), dst[..., :N])
    return xt, yt, Np


def outer_product_ln_linear(x, y, gamma, beta, w, b, eps):
    """Functional form (dispatcher op): x, y 16-bit [B, N, L, 32], any L >= 1 and N <= 128 -> fp32 [B, L, L, Dout]."""
    xt, yt, _ = outer_operands(x, y, x.dtype, outer_depth(x.shape[1]) or 8)   # (N > 128: the kernel refuses the depth)
    wp, s, c = outer_fold(w, gamma, beta, b, x.dtype)
    out = torch.empty(x.shape[0], x.shape[2], x.shape[2], w.shape[0], device=x.device, dtype=F32)
    return outer_fused(xt, yt, wp, s, c, out, eps)


def poswise_collapsed(xn, u, scale):
    """w[b,h,n,l] = softmax_n(scale * xn[b,n,l,:] . u[b,l,h,:]); xn bf16 [B,N,L,D], u bf16 [B,L,H,D] -> fp32 [B,H,N,L]."""
    B, N, L_, D = xn.shape
    H = u.shape[2]
    _need_cuda(xn, u)
    w = torch.empty(B, H, N, L_, device=xn.device, dtype=F32)
    check(lib.rf_poswise_collapsed(ptr(xn), ptr(u), ptr(w), B, N, L_, D, H, float(scale), stream()), "rf_poswise_collapsed")
    return w


def tied_softmax(logits, att, att_sym=None, sym_ld=0):
    """att = softmax over the last dim of fp32 logits [B, H, L, L] (+ the symmetrised map); att [B, H, L, L], or
    [B, H, L, att_ld] with att_ld a multiple of 8 above L: the pad columns are written as zeros (rf_tied_softmax_ld)."""
    B, H, L_, _ = logits.shape
    _need_cuda(logits, att, att_sym)
    if att.shape[-1] != L_:
        check(lib.rf_tied_softmax_ld(ptr(logits), ptr(att), dcode(att.dtype), _att_ld(att, L_), ptr(att_sym), sym_ld, B, H, L_,
                                     stream()), "rf_tied_softmax_ld")
        return
    check(lib.rf_tied_softmax(ptr(logits), ptr(att), dcode(att.dtype), ptr(att_sym), sym_ld, B, H, L_, stream()),
          "rf_tied_softmax")


def poswise(q0, q0_ld, k, k_ld, k_col0, k_hs, dlen, w, q_scale, qs_ld, qs_col0, qs_dh, B, N, L_, H, scale, qscale):
    _need_cuda(q0, k, w, q_scale)
    check(lib.rf_poswise(ptr(q0), dcode(q0.dtype), q0_ld, ptr(k), k_ld, k_col0, k_hs, dlen, ptr(w), ptr(q_scale),
                         qs_ld, qs_col0, qs_dh, dcode(k.dtype), B, N, L_, H, scale, qscale, stream()), "rf_poswise")


def weighted_msa_sum(x, w, y, y_ld):
    B, N, L_, D = x.shape
    _need_cuda(x, w, y)
    check(lib.rf_weighted_msa_sum(ptr(x), dcode(x.dtype), ptr(w), ptr(y), y_ld, B, N, L_, D, stream()),
          "rf_weighted_msa_sum")


def instnorm(x, gamma, beta, *, eps=1e-6, residual=None, act=L.ACT_NONE, out_dtype=None, out2_dtype=None, row_group=None,
             rows_global=None, out=None, out2=None, stats_out=None):
    """InstanceNorm2d(affine) over NHWC x [B,H,W,C]; returns (y, y2) where y2 is an optional second copy.
    row_group / rows_global: x is a block of H of the picture's rows_global rows, the other blocks live on the other ranks of
    the torch.distributed group: the per-(b, c) sums are all-reduced (2*B*C doubles) before they are applied.
    stats_out: a list the fp64 sums of rf_instnorm_stats are appended to (what instnorm_bwd takes)."""
    B, H, W, Cc = x.shape
    _need_cuda(x, gamma, beta, residual)
    sums = torch.empty(B * Cc * 2, device=x.device, dtype=torch.float64)  # fully written by the ordered finalize step
    ws_bytes = int(lib.rf_instnorm_ws_bytes(B, H * W, Cc))  # atomics-free, bitwise reproducible statistics
    ws = torch.empty(ws_bytes, device=x.device, dtype=torch.uint8)
    check(lib.rf_instnorm_stats(ptr(x), dcode(x.dtype), ptr(sums), B, H * W, Cc, ptr(ws), ws_bytes, stream()),
          "rf_instnorm_stats")
    if row_group is not None:
        from . import shard
        shard.all_reduce_sum(sums, row_group)
        # rf_instnorm_apply divides by ITS pixel count: hand it global sums scaled to the local block (exact up to one rounding)
        sums.mul_(float(H) / float(rows_global))
    if stats_out is not None:
        stats_out.append(sums)
    # out / out2: caller-owned contiguous destinations (e.g. the interior of a pre-haloed picture, shard.haloed_buffer)
    y = out if out is not None else torch.empty(x.shape, device=x.device, dtype=out_dtype or x.dtype)
    y2 = out2 if out2 is not None else (torch.empty(x.shape, device=x.device, dtype=out2_dtype) if out2_dtype is not None else None)
    for t in (y, y2):
        if t is not None and (tuple(t.shape) != tuple(x.shape) or not t.is_contiguous()):
            raise ValueError("instnorm: out / out2 must be contiguous tensors of the input's shape")
    _need_cuda(y, y2)
    check(lib.rf_instnorm_apply(ptr(x), dcode(x.dtype), ptr(sums), ptr(gamma), ptr(beta), eps, ptr(residual), act,
                                ptr(y), dcode(y.dtype), ptr(y2), dcode(y2.dtype) if y2 is not None else 0, B, H * W,
                                Cc, stream()), "rf_instnorm_apply")
    return y, y2


# --------------------------------------------------------------------------------------------- backward (csrc/backward.hip)
def conv_wgrad(dy, x, taps, dilation=1, *, bias=False, alpha=1.0):
    """Weight gradient of a stride-1 "same" convolution (rf_conv_wgrad): dy [..., Co], x [..., Ci] contiguous of one dtype
    (fp32: exact; the 16-bit type: MFMA with fp32 accumulation).  taps = 9: NHWC [B, H, W, C] tensors, 3x3 kernel of `dilation`;
    taps = 1: any leading shape (1x1 convolution / Linear over the rows).  Returns (fp32 dW [Co, taps * Ci] in the forward's
    [co][tap][ci] weight layout, fp32 dbias [Co] or None), both times alpha."""
    _need_cuda(dy, x)
    if dy.dtype != x.dtype or not (dy.is_contiguous() and x.is_contiguous()) or dy.shape[:-1] != x.shape[:-1]:
        raise ValueError("conv_wgrad: contiguous dy / x of one dtype and the same pixels")
    Co, Ci = dy.shape[-1], x.shape[-1]
    if taps == 9:
        B, H, W = dy.shape[0], dy.shape[1], dy.shape[2]
    else:
        B, H, W = 1, 1, dy.numel() // Co
    code = dcode(dy.dtype)
    ws_bytes = int(lib.rf_conv_wgrad_ws_bytes(code, B, H, W, Co, Ci, taps))
    if ws_bytes <= 0:
        raise ValueError(f"conv_wgrad: unsupported shape / taps ({tuple(dy.shape)}, {Ci}, taps={taps})")
    ws = torch.empty(ws_bytes, device=dy.device, dtype=torch.uint8)
    dw = torch.empty(Co, taps * Ci, device=dy.device, dtype=F32)
    db = torch.empty(Co, device=dy.device, dtype=F32) if bias else None
    check(lib.rf_conv_wgrad(ptr(dy), ptr(x), code, ptr(dw), ptr(db), B, H, W, Co, Ci, taps, int(dilation), float(alpha), ptr(ws),
                            ws_bytes, stream()), "rf_conv_wgrad")
    return dw, db


def instnorm_bwd(g, x, sums, gamma, *, eps=1e-6, act_out=None, dx_dtype=F32, ge_out=None):
    """InstanceNorm2d(affine) backward over NHWC (rf_instnorm_bwd): g fp32 gradient of the (ELU'd, when act_out = the saved ELU
    output is given) norm output, x the saved norm input, sums the forward's statistics (instnorm(stats_out=...)).
    Returns (dx of dx_dtype, fp32 dgamma [C], fp32 dbeta [C]); ge_out: fp32 destination of g times the ELU derivative (may be g)."""
    B, H, W, Cc = x.shape
    _need_cuda(g, x, sums, gamma, act_out, ge_out)
    for t in (g, x, act_out, ge_out):
        if t is not None and (tuple(t.shape) != tuple(x.shape) or not t.is_contiguous()):
            raise ValueError("instnorm_bwd: contiguous tensors of one shape")
    if g.dtype != F32 or (ge_out is not None and ge_out.dtype != F32):
        raise TypeError("instnorm_bwd: g / ge_out must be fp32")
    ws_bytes = (int(lib.rf_instnorm_ws_bytes(B, H * W, Cc)) + 15) // 16 * 16 + 16 * B * Cc
    ws = torch.empty(ws_bytes, device=x.device, dtype=torch.uint8)
    dx = torch.empty(x.shape, device=x.device, dtype=dx_dtype)
    dgamma = torch.empty(Cc, device=x.device, dtype=F32)
    dbeta = torch.empty(Cc, device=x.device, dtype=F32)
    check(lib.rf_instnorm_bwd(ptr(g), ptr(act_out), dcode(act_out.dtype) if act_out is not None else 0, ptr(x), dcode(x.dtype),
                              ptr(sums), ptr(gamma), float(eps), ptr(dx), dcode(dx_dtype), ptr(ge_out), ptr(dgamma), ptr(dbeta),
                              B, H * W, Cc, ptr(ws), ws_bytes, stream()), "rf_instnorm_bwd")
    return dx, dgamma, dbeta


def layernorm_bwd(x, g, gamma, *, eps=1e-5, dx_dtype=F32):
    """LayerNorm backward over the last dim (rf_layernorm_bwd): x fp32 (the forward's input), g fp32 gradient of the output.
    Returns (dx of dx_dtype, fp32 dgamma [D], fp32 dbeta [D])."""
    D = x.shape[-1]
    rows = x.numel() // D
    _need_cuda(x, g, gamma)
    if x.dtype != F32 or g.dtype != F32 or tuple(g.shape) != tuple(x.shape) or not (x.is_contiguous() and g.is_contiguous()):
        raise ValueError("layernorm_bwd: contiguous fp32 x and g of one shape")
    ws_bytes = int(lib.rf_layernorm_bwd_ws_bytes(rows, D))
    ws = torch.empty(ws_bytes, device=x.device, dtype=torch.uint8)
    dx = torch.empty(x.shape, device=x.device, dtype=dx_dtype)
    dgamma = torch.empty(D, device=x.device, dtype=F32)
    dbeta = torch.empty(D, device=x.device, dtype=F32)
    check(lib.rf_layernorm_bwd(ptr(x), ptr(g), ptr(gamma), float(eps), ptr(dx), dcode(dx_dtype), ptr(dgamma), ptr(dbeta), rows, D,
                               ptr(ws), ws_bytes, stream()), "rf_layernorm_bwd")
    return dx, dgamma, dbeta


def layernorm_bwd_fused(x, g, gamma, beta, *, eps=1e-5, dx=None, z=None, dgamma=None, dbeta=None):
    """LayerNorm forward and backward over the last dim in one pass (rf_layernorm_bwd_fused): x, g contiguous of one shape and
    one dtype (fp32 or the 16-bit type); statistics recomputed in fp32.  Returns (dx, z = LN(x), fp32 dgamma [D], fp32 dbeta [D]),
    dx and z in the operands' dtype.  dx= / z= name the destinations (dx may be g, z may be x); dgamma= / dbeta= given: the
    column sums are ADDED to them (a tensor walked in pieces, in the caller's order)."""
    D = x.shape[-1]
    rows = x.numel() // D
    dx = torch.empty(x.shape, device=x.device, dtype=x.dtype) if dx is None else dx
    z = torch.empty(x.shape, device=x.device, dtype=x.dtype) if z is None else z
    _need_cuda(x, g, gamma, beta, dx, z, dgamma, dbeta)
    for t in (g, dx, z):
        if t.dtype != x.dtype or tuple(t.shape) != tuple(x.shape) or not (t.is_contiguous() and x.is_contiguous()):
            raise ValueError("layernorm_bwd_fused: contiguous x, g, dx and z of one shape and one dtype")
    if (dgamma is None) != (dbeta is None):
        raise ValueError("layernorm_bwd_fused: pass both dgamma and dbeta to accumulate, or neither")
    for t in (gamma, beta, dgamma, dbeta):
        if t is not None and (t.dtype != F32 or t.numel() != D or not t.is_contiguous()):
            raise ValueError("layernorm_bwd_fused: contiguous fp32 gamma / beta / dgamma / dbeta of D elements")
    acc = dgamma is not None
    if not acc:
        dgamma = torch.empty(D, device=x.device, dtype=F32)
        dbeta = torch.empty(D, device=x.device, dtype=F32)
    ws_bytes = int(lib.rf_layernorm_bwd_fused_ws_bytes(rows, D))
    if ws_bytes <= 0:
        raise ValueError(f"layernorm_bwd_fused: unsupported shape {tuple(x.shape)}")
    ws = torch.empty(ws_bytes, device=x.device, dtype=torch.uint8)
    check(lib.rf_layernorm_bwd_fused(ptr(x), ptr(g), dcode(x.dtype), ptr(gamma), ptr(beta), float(eps), ptr(dx), ptr(z), ptr(dgamma),
                                     ptr(dbeta), int(acc), rows, D, ptr(ws), ws_bytes, stream()), "rf_layernorm_bwd_fused")
    return dx, z, dgamma, dbeta


def absmax(xs):
    """max |x| over fp32 tensors (rf_absmax; one host read for the whole list)."""
    _need_cuda(*xs)
    out = torch.empty(len(xs), device=xs[0].device, dtype=F32)
    ws = torch.empty(4096, device=xs[0].device, dtype=torch.uint8)
    for i, x in enumerate(xs):
        if x.dtype != F32 or not x.is_contiguous():
            raise ValueError("absmax: contiguous fp32 tensors")
        check(lib.rf_absmax(ptr(x), x.numel(), ptr(out, i), ptr(ws), 4096, stream()), "rf_absmax")
    return max(out.tolist())


def linattn_normalize_bwd(num, num_ld, g, g_ld, dnum, dnum_ld, rows, dh):
    """Backward of linattn_normalize (rf_linattn_normalize_bwd): num fp32 rows (column dh = the denominator), g fp32 gradient of
    the normalised rows; writes dnum (fp32 / the 16-bit type): g / den in columns < dh, -sum g out / den in column dh, zeros up
    to dnum_ld."""
    _need_cuda(num, g, dnum)
    if num.dtype != F32 or g.dtype != F32:
        raise TypeError("linattn_normalize_bwd: num and g must be fp32")
    check(lib.rf_linattn_normalize_bwd(ptr(num), int(num_ld), ptr(g), int(g_ld), ptr(dnum), dcode(dnum.dtype), int(dnum_ld), int(rows),
                                       int(dh), stream()), "rf_linattn_normalize_bwd")
    return dnum


def relu_feature_bwd(dphi, z, nvalid, out_dtype):
    """Backward of the ReLU feature map relu(z) + eps (rf_relu_feature_bwd): dphi, z contiguous fp32 [..., ld] (z the fp32
    pre-activation); returns dphi * 1[z > 0] in columns < nvalid, 0 beyond, as out_dtype."""
    _need_cuda(dphi, z)
    if dphi.dtype != F32 or z.dtype != F32 or dphi.shape != z.shape or not (dphi.is_contiguous() and z.is_contiguous()):
        raise ValueError("relu_feature_bwd: contiguous fp32 dphi and z of one shape")
    ld = dphi.shape[-1]
    dz = torch.empty(dphi.shape, device=dphi.device, dtype=out_dtype)
    check(lib.rf_relu_feature_bwd(ptr(dphi), ptr(z), ptr(dz), dcode(out_dtype), dphi.numel() // ld, ld, int(nvalid), stream()),
          "rf_relu_feature_bwd")
    return dz


def relu_dropout_bwd(g, hpre, out_dtype, drop=None):
    """Backward of dropout(relu(hpre)) (rf_relu_dropout_bwd): g, hpre contiguous fp32 of one shape; drop = (p, seed, offset) of
    the forward's rf_dropout mask or None.  Returns g * 1[hpre > 0] (* mask / (1 - p)) as out_dtype."""
    _need_cuda(g, hpre)
    if g.dtype != F32 or hpre.dtype != F32 or g.shape != hpre.shape or not (g.is_contiguous() and hpre.is_contiguous()):
        raise ValueError("relu_dropout_bwd: contiguous fp32 g and hpre of one shape")
    p, seed, off = drop if drop is not None else (0.0, 0, 0)
    dh = torch.empty(g.shape, device=g.device, dtype=out_dtype)
    if p >= 1.0:
        return fill(dh, 0.0)
    check(lib.rf_relu_dropout_bwd(ptr(g), ptr(hpre), ptr(dh), dcode(out_dtype), float(p), int(seed), int(off), g.numel(), stream()),
          "rf_relu_dropout_bwd")
    return dh


def graph_attention_bwd(q, k, v, e, g, B, L_, H, d, scale, dropout=None, mask=None):
    """Backward of graph_attention in any of its forms (rf_graph_attention_bwd): q, k, v [B, L, H*d] and e [B, L, L, H*d] the
    forward's operands (contiguous, one dtype), g contiguous fp32 [B, L, H*d] = d out; dropout = the forward's (p, seed, offset)
    or None; mask = the forward's uint8 [B, L, L] or None.  Returns (dq, dk, dv fp32 [B, L, H*d], de [B, L, L, H*d] in the
    operands' dtype, pd, ds fp32 [B, H, L, L]): pd the probabilities after dropout, ds the logits' gradient, both exactly 0 at a
    masked column, like de.  A row with no edge: dq = 0, ds = 0, de = pd g with p = 1 / L -- the derivative of the uniform
    attention the forward computes there (the reference's autograd differentiates logits its own -1e9 rounds away)."""
    _need_cuda(q, k, v, e, g, mask)
    HD = H * d
    for t_ in (q, k, v):
        if t_.dtype != e.dtype or tuple(t_.shape) != (B, L_, HD) or not t_.is_contiguous():
            raise ValueError(f"graph_attention_bwd: contiguous q, k, v [{B}, {L_}, {HD}] of e's dtype")
    if tuple(e.shape) != (B, L_, L_, HD) or not e.is_contiguous():
        raise ValueError(f"graph_attention_bwd: contiguous e [{B}, {L_}, {L_}, {HD}]")
    if g.dtype != F32 or tuple(g.shape) != (B, L_, HD) or not g.is_contiguous():
        raise ValueError(f"graph_attention_bwd: contiguous fp32 g [{B}, {L_}, {HD}]")
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (B, L_, L_) or not mask.is_contiguous()):
        raise ValueError(f"mask must be a contiguous uint8 [{B}, {L_}, {L_}] tensor, got {mask.dtype} {tuple(mask.shape)}")
    pd_, seed, off = dropout if dropout is not None else (0.0, 0, 0)
    dev = q.device
    dq, dk, dv = (torch.empty(B, L_, HD, device=dev, dtype=F32) for _ in range(3))
    de = torch.empty(B, L_, L_, HD, device=dev, dtype=e.dtype)
    pmap, smap = (torch.empty(B, H, L_, L_, device=dev, dtype=F32) for _ in range(2))
    check(lib.rf_graph_attention_bwd(ptr(q), ptr(k), ptr(v), ptr(e), dcode(e.dtype), ptr(mask), ptr(g), ptr(dq), ptr(dk), ptr(dv),
                                     ptr(de), ptr(pmap), ptr(smap), L_, B, L_, H, d, scale, float(pd_), int(seed), int(off),
                                     stream()), "rf_graph_attention_bwd")
    return dq, dk, dv, de, pmap, smap


def elu_bwd(g, y, x, out_dtype):
    """ELU backward from the activation's value (rf_elu_bwd): g, y (and x, or None) contiguous fp32 of one shape, y = x + ELU(z).
    Returns g * (a > 0 ? 1 : a + 1) with a = y - x, as out_dtype."""
    _need_cuda(g, y, x)
    for t_ in (g, y, x):
        if t_ is not None and (t_.dtype != F32 or t_.shape != g.shape or not t_.is_contiguous()):
            raise ValueError("elu_bwd: contiguous fp32 g, y and x of one shape")
    da = torch.empty(g.shape, device=g.device, dtype=out_dtype)
    check(lib.rf_elu_bwd(ptr(g), ptr(y), ptr(x), ptr(da), dcode(out_dtype), g.numel(), stream()), "rf_elu_bwd")
    return da


def poswise_bwd(q0, q0_ld, k, k_ld, k_col0, k_hs, dlen, B, N, L_, H, scale, *, dw=None, ds=None, ds_ld=None, dk=None,
                dk_dtype=F32, dk_ld=None, dk_col0=0, dk_hs=None, dropout=None):
    """Backward of poswise in its addressing (rf_poswise_bwd): q0 rows [B*L] of q0_ld, k rows [B*N*L] of k_ld with head h at column
    k_col0 + h * k_hs (dlen columns); dw contiguous fp32 [B, N, H, L] = the gradient of the weights (after their dropout) or None;
    ds fp32 rows [B*L] of ds_ld = the gradient of sum_n w_n k_n (weighted_msa_sum fused behind the weights: the collapsed form,
    H == 1) or None; dropout = the forward's (p, seed, offset) on the weights or None.  Returns (dq0 fp32 [B, L, H * dlen], dk):
    dk = the given tensor (rows of dk_ld, head h at column dk_col0 + h * dk_hs), or a new contiguous [B, N, L, H * dlen] of
    dk_dtype."""
    _need_cuda(q0, k, dw, ds, dk)
    HD = H * dlen
    if min(B, N, L_, H, dlen) <= 0 or min(k_col0, k_hs, dk_col0) < 0:
        raise ValueError("poswise_bwd: sizes must be positive, offsets and strides non-negative")
    if dk is None:
        dk = torch.empty(B, N, L_, HD, device=k.device, dtype=dk_dtype)
        dk_ld, dk_col0, dk_hs = HD, 0, dlen
    elif dk_ld is None or dk_hs is None:
        raise ValueError("poswise_bwd: a given dk needs dk_ld and dk_hs")
    if dw is None and ds is None:
        raise ValueError("poswise_bwd: dw or ds (or both)")
    for t_ in (q0, k, dk):
        if not t_.is_contiguous():
            raise ValueError("poswise_bwd: contiguous q0, k and dk")
    if q0_ld < HD or q0.numel() < (B * L_ - 1) * q0_ld + HD:
        raise ValueError(f"poswise_bwd: q0 holds {q0.numel()} elements, too few for [{B * L_}] rows of {q0_ld} with {HD} columns")
    rows = B * N * L_
    if k_ld < k_col0 + (H - 1) * k_hs + dlen or k.numel() < (rows - 1) * k_ld + k_col0 + (H - 1) * k_hs + dlen:
        raise ValueError(f"poswise_bwd: k holds {k.numel()} elements, too few for [{rows}] rows of {k_ld}")
    if (dk_ld < dk_col0 + (H - 1) * dk_hs + dlen or (H > 1 and dk_hs < dlen)
            or dk.numel() < (rows - 1) * dk_ld + dk_col0 + (H - 1) * dk_hs + dlen):
        raise ValueError(f"poswise_bwd: dk holds {dk.numel()} elements, too few for [{rows}] rows of {dk_ld}")
    if dw is not None and (dw.dtype != F32 or dw.numel() != B * N * H * L_ or not dw.is_contiguous()):
        raise ValueError(f"poswise_bwd: contiguous fp32 dw [{B}, {N}, {H}, {L_}]")
    if ds is not None:
        ds_ld = dlen if ds_ld is None else ds_ld
        if H != 1:
            raise ValueError("poswise_bwd: ds goes with the collapsed one-head form (H == 1)")
        if ds.dtype != F32 or not ds.is_contiguous() or ds_ld < dlen or ds.numel() < (B * L_ - 1) * ds_ld + dlen:
            raise ValueError(f"poswise_bwd: contiguous fp32 ds, [{B * L_}] rows of {ds_ld} with {dlen} columns")
    p, seed, off = dropout if dropout is not None else (0.0, 0, 0)
    dq0 = torch.empty(B, L_, HD, device=k.device, dtype=F32)
    if p >= 1.0:   # everything was dropped: the weights, and with them both gradients, are zero
        fill(dq0, 0.0)
        if dk_ld == HD and dk_col0 == 0 and (H == 1 or dk_hs == dlen):
            return dq0, fill(dk, 0.0)
        raise ValueError("poswise_bwd: p >= 1 with a strided dk")
    check(lib.rf_poswise_bwd(ptr(q0), dcode(q0.dtype), int(q0_ld), ptr(k), dcode(k.dtype), int(k_ld), int(k_col0), int(k_hs),
                             int(dlen), ptr(dw), ptr(ds), int(ds_ld or 0), ptr(dq0), ptr(dk), dcode(dk.dtype), int(dk_ld),
                             int(dk_col0), int(dk_hs), B, N, L_, H, float(scale), float(p), int(seed), int(off), stream()),
          "rf_poswise_bwd")
    return dq0, dk


def tied_softmax_bwd(logits, dp, g_sym=None, h16_copies=False):
    """Backward of tied_softmax and of its symmetrised map (rf_tied_softmax_bwd): logits and dp (the value-path part of the
    probabilities' gradient) contiguous fp32 [B, H, L, L]; g_sym contiguous fp32 [B, L, L, H], the gradient of the symmetrised
    map, or None.  Returns (ds fp32 [B, H, L, L], p, ds16): with h16_copies the probabilities and ds in the active library's
    16-bit type, [B, H, L, tied_ld(L)] with zeros in the pad columns (16-bit GEMM operands at any L); else (ds, None, None)."""
    _need_cuda(logits, dp, g_sym)
    if logits.dim() != 4 or logits.shape[2] != logits.shape[3]:
        raise ValueError("tied_softmax_bwd: logits [B, H, L, L]")
    B, H, L_, _ = logits.shape
    for t_ in (logits, dp):
        if t_.dtype != F32 or tuple(t_.shape) != (B, H, L_, L_) or not t_.is_contiguous():
            raise ValueError(f"tied_softmax_bwd: contiguous fp32 logits and dp [{B}, {H}, {L_}, {L_}]")
    if g_sym is not None and (g_sym.dtype != F32 or tuple(g_sym.shape) != (B, L_, L_, H) or not g_sym.is_contiguous()):
        raise ValueError(f"tied_softmax_bwd: contiguous fp32 g_sym [{B}, {L_}, {L_}, {H}]")
    ds = torch.empty(B, H, L_, L_, device=logits.device, dtype=F32)
    ld_ = tied_ld(L_)
    p16 = torch.empty(B, H, L_, ld_, device=logits.device, dtype=h16()) if h16_copies else None
    ds16 = torch.empty(B, H, L_, ld_, device=logits.device, dtype=h16()) if h16_copies else None
    check(lib.rf_tied_softmax_bwd(ptr(logits), ptr(dp), ptr(g_sym), ptr(ds), ptr(p16), ptr(ds16), ld_, B, H, L_, stream()),
          "rf_tied_softmax_bwd")
    return ds, p16, ds16


def scale_rows_bwd(x, x_ld, x_hs, gy, gy_ld, gy_hs, w, alpha, tokens, H, D, *, dx=None, dx_ld=None, dx_hs=None, dx_dtype=None,
                   want_dw=True, x_off=0, gy_off=0, dx_off=0):
    """Backward of y[r, :] = alpha * w[r] * x[r, :] (rf_scale_rows_bwd) over rows r = (t, h), t < tokens, h < H, of D columns:
    row (t, h) of x starts at element x_off + t * x_ld + h * x_hs, likewise gy (the gradient of y) and dx; w contiguous fp32
    [tokens * H].  Returns (dx = alpha * w * gy: the given tensor, or a new contiguous [tokens, H * D] of dx_dtype (default:
    gy's), fp32 dw [tokens * H] = alpha * sum_c gy * x, or None)."""
    _need_cuda(x, gy, w, dx)
    if min(tokens, H, D) <= 0 or min(x_ld, x_hs, gy_ld, gy_hs, x_off, gy_off, dx_off) < 0:
        raise ValueError("scale_rows_bwd: sizes must be positive, offsets and strides non-negative")
    if dx is None:
        dx = torch.empty(tokens, H * D, device=gy.device, dtype=dx_dtype or gy.dtype)
        dx_ld, dx_hs, dx_off = H * D, D, 0
    elif dx_ld is None or dx_hs is None or min(dx_ld, dx_hs) < 0:
        raise ValueError("scale_rows_bwd: a given dx needs dx_ld and dx_hs")
    for name, t_, off, ld_, hs in (("x", x, x_off, x_ld, x_hs), ("gy", gy, gy_off, gy_ld, gy_hs), ("dx", dx, dx_off, dx_ld, dx_hs)):
        if not t_.is_contiguous() or t_.numel() < off + (tokens - 1) * ld_ + (H - 1) * hs + D:
            raise ValueError(f"scale_rows_bwd: {name} holds {t_.numel()} elements, too few for [{tokens}, {H}] rows of {D} "
                             f"at strides ({ld_}, {hs}) from {off} (or is not contiguous)")
    if w.dtype != F32 or w.numel() != tokens * H or not w.is_contiguous():
        raise ValueError(f"scale_rows_bwd: contiguous fp32 w [{tokens * H}]")
    dw = torch.empty(tokens * H, device=gy.device, dtype=F32) if want_dw else None
    check(lib.rf_scale_rows_bwd(ptr(x, x_off), dcode(x.dtype), int(x_ld), int(x_hs), ptr(gy, gy_off), dcode(gy.dtype), int(gy_ld),
                                int(gy_hs), ptr(w), float(alpha), ptr(dx, dx_off), dcode(dx.dtype), int(dx_ld), int(dx_hs),
                                ptr(dw), int(tokens), int(H), int(D), stream()), "rf_scale_rows_bwd")
    return dx, dw


def pair_softmax_bwd(logits, datt, nz_pad=None):
    """Backward of the batched per-(layer, head) softmax of MsaUpdateWithPair's shared front (rf_pair_softmax_bwd): logits
    contiguous fp32 [B, L, L, NZ] (what softmax_batched read), datt contiguous fp32 [NZ, B, L, ld >= L], the gradient of the
    maps (columns past L are not read).  Returns (dz fp32 [B, L, L, NZ], dz16): with nz_pad (a multiple of 8, >= NZ) the same
    gradient in the active library's 16-bit type, [B, L, L, nz_pad] with zeros in the pad columns (rf_conv_wgrad's dy operand);
    else (dz, None)."""
    _need_cuda(logits, datt)
    if logits.dim() != 4 or logits.shape[1] != logits.shape[2] or logits.dtype != F32 or not logits.is_contiguous():
        raise ValueError("pair_softmax_bwd: contiguous fp32 logits [B, L, L, NZ]")
    B, L_, _, NZ = logits.shape
    if datt.dim() != 4 or datt.dtype != F32 or tuple(datt.shape[:3]) != (NZ, B, L_) or datt.shape[3] < L_ or not datt.is_contiguous():
        raise ValueError(f"pair_softmax_bwd: contiguous fp32 datt [{NZ}, {B}, {L_}, >= {L_}]")
    if nz_pad is not None and (nz_pad < NZ or nz_pad % 8):
        raise ValueError(f"pair_softmax_bwd: nz_pad must be a multiple of 8 and at least {NZ}, got {nz_pad}")
    dz = torch.empty(B, L_, L_, NZ, device=logits.device, dtype=F32)
    dz16 = torch.empty(B, L_, L_, nz_pad, device=logits.device, dtype=h16()) if nz_pad is not None else None
    check(lib.rf_pair_softmax_bwd(ptr(logits), ptr(datt), int(datt.shape[3]), ptr(dz), ptr(dz16), int(nz_pad or 0), B, L_, NZ,
                                  stream()), "rf_pair_softmax_bwd")
    return dz, dz16


def sym_layernorm_bwd(pair, dz, w, eps=1e-5):
    """Backward of sym_layernorm(pair) @ w^T (rf_sym_layernorm_bwd): pair contiguous fp32 [B, L, L, D], dz contiguous fp32
    [B, L, L, NZ], w contiguous fp32 [NZ, D] (the projection with the LayerNorm's gamma folded in).  Returns fp32 d pair."""
    _need_cuda(pair, dz, w)
    if pair.dim() != 4 or pair.shape[1] != pair.shape[2] or pair.dtype != F32 or not pair.is_contiguous():
        raise ValueError("sym_layernorm_bwd: contiguous fp32 pair [B, L, L, D]")
    B, L_, _, D = pair.shape
    if w.dim() != 2 or w.shape[1] != D or w.dtype != F32 or not w.is_contiguous():
        raise ValueError(f"sym_layernorm_bwd: contiguous fp32 w [NZ, {D}]")
    NZ = w.shape[0]
    if dz.dtype != F32 or tuple(dz.shape) != (B, L_, L_, NZ) or not dz.is_contiguous():
        raise ValueError(f"sym_layernorm_bwd: contiguous fp32 dz [{B}, {L_}, {L_}, {NZ}]")
    dpair = torch.empty(pair.shape, device=pair.device, dtype=F32)
    check(lib.rf_sym_layernorm_bwd(ptr(pair), ptr(dz), ptr(w), ptr(dpair), B, L_, D, NZ, float(eps), stream()),
          "rf_sym_layernorm_bwd")
    return dpair


def embedding_bwd(idx, g, n_rows, *, query=None, drop=None):
    """Gradient of an embedding table of n_rows rows (rf_embedding_bwd): idx contiguous int64 of any shape, g contiguous fp32
    [*idx.shape, D], the gradient of the embedded tensor.  drop = (p, seed, offset): the forward's dropout mask over that tensor,
    replayed inside the kernel (None: no dropout).  query = (N, L): also the gradient of the two query-encoding rows from the
    unmasked g, the rows being [.., N, L] (first MSA row / the others).  Returns (fp32 [n_rows, D], fp32 [2, D] or None)."""
    _need_cuda(idx, g)
    D = g.shape[-1]
    rows = idx.numel()
    if (idx.dtype != torch.int64 or g.dtype != F32 or tuple(g.shape[:-1]) != tuple(idx.shape)
            or not (idx.is_contiguous() and g.is_contiguous())):
        raise ValueError("embedding_bwd: contiguous int64 idx [...] and fp32 g [..., D]")
    p, seed, off = drop if drop is not None else (0.0, 0, 0)
    N, L_ = query if query is not None else (1, 1)
    ws_bytes = int(lib.rf_embedding_bwd_ws_bytes(rows, D, int(n_rows)))
    if ws_bytes <= 0:
        raise ValueError(f"embedding_bwd: unsupported problem ({rows} rows, D = {D}, a table of {n_rows} rows)")
    ws = torch.empty(ws_bytes, device=g.device, dtype=torch.uint8)
    dtable = torch.empty(n_rows, D, device=g.device, dtype=F32)
    dq = torch.empty(2, D, device=g.device, dtype=F32) if query is not None else None
    check(lib.rf_embedding_bwd(ptr(idx), ptr(g), ptr(dtable), ptr(dq), rows, D, int(n_rows), int(N), int(L_), float(p), int(seed),
                               int(off), ptr(ws), ws_bytes, stream()), "rf_embedding_bwd")
    return dtable, dq


def pair_axis_sums(g, aa_idx):
    """The sums of a pair-shaped gradient over each picture axis (rf_pair_axis_sums): g contiguous fp32 [B, L, L, D], aa_idx
    contiguous int64 [B, L].  Returns (rows [B, L, D] = sum_j g, cols [B, L, D] = sum_i g, dsep [D] = sum g log(|idx_i - idx_j| + 1),
    dbias [D] = sum g), all fp32."""
    _need_cuda(g, aa_idx)
    if g.dim() != 4 or g.shape[1] != g.shape[2] or g.dtype != F32 or not g.is_contiguous():
        raise ValueError("pair_axis_sums: contiguous fp32 g [B, L, L, D]")
    B, L_, _, D = g.shape
    if aa_idx.dtype != torch.int64 or tuple(aa_idx.shape) != (B, L_) or not aa_idx.is_contiguous():
        raise ValueError(f"pair_axis_sums: contiguous int64 aa_idx [{B}, {L_}]")
    ws_bytes = int(lib.rf_pair_axis_sums_ws_bytes(B, L_, D))
    if ws_bytes <= 0:
        raise ValueError(f"pair_axis_sums: unsupported shape {tuple(g.shape)}")
    ws = torch.empty(ws_bytes, device=g.device, dtype=torch.uint8)
    rows = torch.empty(B, L_, D, device=g.device, dtype=F32)
    cols = torch.empty(B, L_, D, device=g.device, dtype=F32)
    dsep = torch.empty(D, device=g.device, dtype=F32)
    dbias = torch.empty(D, device=g.device, dtype=F32)
    check(lib.rf_pair_axis_sums(ptr(g), ptr(aa_idx), ptr(rows), ptr(cols), ptr(dsep), ptr(dbias), B, L_, D, ptr(ws), ws_bytes,
                                stream()), "rf_pair_axis_sums")
    return rows, cols, dsep, dbias


def center_channels(x, out=None):
    """y[b, i, j, c] = x[b, i, j, c] - mean_{i,j} x[b, :, :, c]  (fp32 NHWC, in place by default): rf_instnorm_stats + the
    centre-only form of rf_instnorm_apply (gamma = beta = NULL).  Exact in front of anything an InstanceNorm follows through
    per-channel-linear maps (1x1 convolution -> InstanceNorm is invariant to a per-channel constant of its input)."""
    B, H, W, Cc = x.shape
    _need_cuda(x, out)
    sums = torch.empty(B * Cc * 2, device=x.device, dtype=torch.float64)
    ws_bytes = int(lib.rf_instnorm_ws_bytes(B, H * W, Cc))
    ws = torch.empty(ws_bytes, device=x.device, dtype=torch.uint8)
    check(lib.rf_instnorm_stats(ptr(x), dcode(x.dtype), ptr(sums), B, H * W, Cc, ptr(ws), ws_bytes, stream()), "rf_instnorm_stats")
    y = x if out is None else out
    check(lib.rf_instnorm_apply(ptr(x), dcode(x.dtype), ptr(sums), None, None, 0.0, None, L.ACT_NONE, ptr(y), dcode(y.dtype), None, 0,
                                B, H * W, Cc, stream()), "rf_instnorm_apply")
    return y


def channel_mean(x, row_group=None, rows_global=None):
    """fp32 [B, C] mean over the picture of NHWC x (rf_instnorm_stats + rf_instnorm_mean; row_group / rows_global as in
    instnorm: x is a block of rows of a sharded picture, the sums are all-reduced)."""
    B, H, W, Cc = x.shape
    _need_cuda(x)
    if row_group is None and x.dtype == F32 and Cc % 4 == 0 and Cc <= 1024 and x.is_contiguous():
        ws_bytes = int(lib.rf_channel_mean_ws_bytes(B, H * W, Cc))
        ws = torch.empty(ws_bytes, device=x.device, dtype=torch.uint8)
        mean = torch.empty(B, Cc, device=x.device, dtype=F32)
        check(lib.rf_channel_mean(ptr(x), ptr(mean), B, H * W, Cc, ptr(ws), ws_bytes, stream()), "rf_channel_mean")
        return mean
    sums = torch.empty(B * Cc * 2, device=x.device, dtype=torch.float64)
    ws_bytes = int(lib.rf_instnorm_ws_bytes(B, H * W, Cc))
    ws = torch.empty(ws_bytes, device=x.device, dtype=torch.uint8)
    check(lib.rf_instnorm_stats(ptr(x), dcode(x.dtype), ptr(sums), B, H * W, Cc, ptr(ws), ws_bytes, stream()), "rf_instnorm_stats")
    count = H * W
    if row_group is not None:
        from . import shard
        shard.all_reduce_sum(sums, row_group)
        count = rows_global * W
    mean = torch.empty(B, Cc, device=x.device, dtype=F32)
    check(lib.rf_instnorm_mean(ptr(sums), ptr(mean), B, count, Cc, stream()), "rf_instnorm_mean")
    return mean


def sample_mean(x, nsample=512):
    """fp32 [B, C] estimate of the per-channel mean of x [B, ..., C] (fp32 / 16-bit, contiguous) from nsample evenly spaced rows."""
    B, Cc = x.shape[0], x.shape[-1]
    _need_cuda(x)
    if not x.is_contiguous():
        raise ValueError("sample_mean: contiguous input")
    mean = torch.empty(B, Cc, device=x.device, dtype=F32)
    check(lib.rf_sample_mean(ptr(x), dcode(x.dtype), ptr(mean), B, x.numel() // (B * Cc), Cc, nsample, stream()), "rf_sample_mean")
    return mean


def center_apply(x, mean, out=None, out_dtype=None):
    """out[b, ..., c] = x[b, ..., c] - mean[b, c]; x fp32 [B, ..., C] contiguous, out fp32 (default: in place) or 16-bit."""
    B, Cc = x.shape[0], x.shape[-1]
    y = out if out is not None else (x if out_dtype in (None, F32) else torch.empty(x.shape, device=x.device, dtype=out_dtype))
    _need_cuda(x, mean, y)
    if x.dtype != F32 or not x.is_contiguous() or not y.is_contiguous() or tuple(y.shape) != tuple(x.shape) or tuple(mean.shape) != (B, Cc):
        raise ValueError("center_apply: x fp32 contiguous, out of x's shape and contiguous, mean [B, C]")
    check(lib.rf_center_apply(ptr(x), ptr(mean), ptr(y), dcode(y.dtype), B, x.numel() // (B * Cc), Cc, stream()), "rf_center_apply")
    return y


def center_rows(x):
    """x fp32 [B, R, C] (small): x -= mean over R, in place; returns the fp32 [B, C] mean."""
    B, R, Cc = x.shape
    _need_cuda(x)
    if x.dtype != F32 or not x.is_contiguous():
        raise ValueError("center_rows: fp32 contiguous [B, R, C]")
    mean = torch.empty(B, Cc, device=x.device, dtype=F32)
    check(lib.rf_center_rows(ptr(x), ptr(mean), B, R, Cc, stream()), "rf_center_rows")
    return mean


def fold_mean(w, mean, bias=None, *, k0=0, nseg=1, seg_stride=0, sum_seg=True):
    """The constant's way through a weight matrix (rf_fold_mean): w fp32 [N, ldw], mean fp32 [B, K] ->
    sum_seg: [B, N] = bias + sum_s w[:, k0 + s*seg_stride : +K] @ mean ; else [B, nseg, N], one product per segment."""
    N, ldw = w.shape
    B, K = mean.shape
    _need_cuda(w, mean, bias)
    if w.dtype != F32 or mean.dtype != F32 or not w.is_contiguous() or not mean.is_contiguous():
        raise ValueError("fold_mean: fp32 contiguous operands")
    out = torch.empty((B, N) if sum_seg else (B, nseg, N), device=w.device, dtype=F32)
    check(lib.rf_fold_mean(ptr(w), ldw, k0, K, nseg, seg_stride, 1 if sum_seg else 0, ptr(mean), ptr(bias), ptr(out), B, N,
                           stream()), "rf_fold_mean")
    return out


def conv3x3_border_fix(y, taps, dilation=1, edges=15):
    """y NHWC (fp32 / 16-bit, in place) -= the taps [B, 9, C] that fall outside the picture (rf_conv3x3_border_fix)."""
    B, H, W, Cc = y.shape
    _need_cuda(y, taps)
    if not y.is_contiguous() or tuple(taps.shape) != (B, 9, Cc) or taps.dtype != F32 or not taps.is_contiguous():
        raise ValueError("conv3x3_border_fix: y contiguous NHWC, taps fp32 [B, 9, C]")
    check(lib.rf_conv3x3_border_fix(ptr(y), dcode(y.dtype), ptr(taps), B, H, W, Cc, dilation, edges, stream()), "rf_conv3x3_border_fix")
    return y


# --------------------------------------------------------------------------------------------- misc
def msa_embed(msa, aa_idx, emb, pe, qenc):
    B, N, L_ = msa.shape
    D = emb.shape[1]
    y = torch.empty(B, N, L_, D, device=msa.device, dtype=F32)
    _need_cuda(msa, aa_idx, emb, pe, qenc)
    check(lib.rf_msa_embed(ptr(msa), ptr(aa_idx), ptr(emb), ptr(pe), ptr(qenc), ptr(y), B, N, L_, D, stream()),
          "rf_msa_embed")
    return y


def pair_embed(seq, aa_idx, tl, tr, wsep, bias, pe):
    B, L_ = seq.shape
    D = tl.shape[1]
    y = torch.empty(B, L_, L_, D, device=seq.device, dtype=F32)
    _need_cuda(seq, aa_idx, tl, tr, wsep, bias, pe)
    check(lib.rf_pair_embed(ptr(seq), ptr(aa_idx), ptr(tl), ptr(tr), ptr(wsep), ptr(bias), ptr(pe), ptr(y), B, L_, D,
                            stream()), "rf_pair_embed")
    return y


def copy_walk(shape, src_strides, dst_strides):
    """(dims, xs, ys) of the row-major walk of one copy: dimensions of size 1 dropped, and a dimension merged into its right
    neighbour where both sides step contiguously from one into the other.  The sequence of (source, destination) addresses is
    that of the full shape; only the constants the kernel divides by change.  Host arithmetic on integers only."""
    dims, xs, ys = [], [], []
    for n, sx, sy in zip(shape, src_strides, dst_strides):
        n, sx, sy = int(n), int(sx), int(sy)
        if n == 1:
            continue
        if dims and xs[-1] == sx * n and ys[-1] == sy * n:
            dims[-1], xs[-1], ys[-1] = dims[-1] * n, sx, sy
        else:
            dims.append(n), xs.append(sx), ys.append(sy)
    return tuple(dims), tuple(xs), tuple(ys)


def copy(src, dst):
    """dst.copy_(src) by rf_copy4d between two views of equal shape (any rank that merges to four dimensions; fp32 <-> 16-bit
    converts).  The elements are walked row-major over the views' shape, so the side that carries the permute is the strided
    one.  Returns dst."""
    _need_cuda(src, dst)
    if src.shape != dst.shape:
        raise ValueError(f"copy: shapes differ: {tuple(src.shape)} and {tuple(dst.shape)}")
    dims, xs, ys = copy_walk(src.shape, src.stride(), dst.stride())
    if len(dims) > 4:
        raise ValueError(f"copy: {tuple(src.shape)} with strides {src.stride()} -> {dst.stride()} needs {len(dims)} dimensions")
    if any(n > 1 and s == 0 for n, s in zip(dims, ys)):
        raise ValueError(f"copy: the destination repeats elements (strides {dst.stride()} of shape {tuple(dst.shape)})")
    pad = 4 - len(dims)
    check(lib.rf_copy4d(ptr(src), dcode(src.dtype), _i4((0,) * pad + xs), ptr(dst), dcode(dst.dtype), _i4((0,) * pad + ys),
                        _i4((1,) * pad + dims), stream()), "rf_copy4d")
    return dst


def cast(x, dtype):
    """contiguous copy of x in another dtype."""
    if x.dtype == dtype:
        return x
    y = torch.empty(x.shape, device=x.device, dtype=dtype)
    axpby(x, 1.0, None, 0.0, y)
    return y


def axpby(x, a, z, b, y):
    _need_cuda(x, z, y)
    check(lib.rf_axpby(ptr(x), dcode(x.dtype), a, ptr(z), dcode(z.dtype) if z is not None else 0, b, ptr(y),
                       dcode(y.dtype), x.numel(), stream()), "rf_axpby")
    return y


def favor_softmax_features(dash, x, x_off, xs, n1, n2, S, n, m, m_pad, dh, is_query, transposed, eps=1e-4):
    _need_cuda(dash, x)
    check(lib.rf_favor_softmax_features(ptr(dash), ptr(x, x_off), _i4(xs), n1, n2, ptr(dash), dcode(dash.dtype), S, n,
                                        m, m_pad, dh, is_query, transposed, eps, stream()),
          "rf_favor_softmax_features")


def linattn_normalize(num, num_ld, y, y_ld, rows, dh):
    _need_cuda(num, y)
    check(lib.rf_linattn_normalize(ptr(num), num_ld, ptr(y), dcode(y.dtype), y_ld, rows, dh, stream()),
          "rf_linattn_normalize")


def tile_1d_feats(msa1d, feat, feat_ld, c0, B, L_, P2):
    _need_cuda(msa1d, feat)
    check(lib.rf_tile_1d_feats(ptr(msa1d), ptr(feat), dcode(feat.dtype), feat_ld, c0, B, L_, P2, stream()),
          "rf_tile_1d_feats")


def graph_attention(q, k, v, e, out, B, L_, H, d, scale, dropout=None, mask=None):
    """dropout = (p, seed, offset): the training-mode form (att_dropout on the probabilities, rf.py:658).
    mask: uint8 [B, L, L] on the device, nonzero = the edge (i, j) exists (the reference's edge_mask, rf.py:652-655).  A row takes
    its softmax over its edges only (masked columns: probability exactly 0, their k, v, e are not read); a row with no edge gets
    the uniform 1/L over all columns -- the reference's result whenever every scaled logit lies in (-32, 32), where the float32
    x - 1e9 rounds to -1e9 for all of them (include/rfmi.h: rf_graph_attention_masked).  The work follows each row's degree."""
    _need_cuda(q, k, v, e, out)
    if mask is not None:
        if mask.dtype != torch.uint8 or tuple(mask.shape) != (B, L_, L_) or not mask.is_contiguous():
            raise ValueError(f"mask must be a contiguous uint8 [{B}, {L_}, {L_}] tensor, got {mask.dtype} {tuple(mask.shape)}")
        _need_cuda(mask)
        pd, seed, off = dropout if dropout is not None else (0.0, 0, 0)
        check(lib.rf_graph_attention_masked(ptr(q), ptr(k), ptr(v), ptr(e), dcode(q.dtype), ptr(mask), ptr(out), B, L_, H, d, scale,
                                            float(pd), int(seed), int(off), stream()), "rf_graph_attention_masked")
        return
    if dropout is not None:
        pd, seed, off = dropout
        check(lib.rf_graph_attention_dropout(ptr(q), ptr(k), ptr(v), ptr(e), dcode(q.dtype), ptr(out), B, L_, H, d, scale,
                                             float(pd), int(seed), int(off), stream()), "rf_graph_attention_dropout")
        return
    check(lib.rf_graph_attention(ptr(q), ptr(k), ptr(v), ptr(e), dcode(q.dtype), ptr(out), B, L_, H, d, scale,
                                 stream()), "rf_graph_attention")


def dropout(x, p, seed, offset, out=None):
    """nn.Dropout of the training-mode forward (rf_dropout): out[e] = keep ? x[e] / (1 - p) : 0 with the Philox mask
    (seed, offset); in place by default.  fp32 / 16-bit contiguous tensors."""
    y = x if out is None else out
    _need_cuda(x, y)
    if not (x.is_contiguous() and y.is_contiguous()) or x.dtype != y.dtype:
        raise ValueError("dropout: contiguous tensors of one dtype")
    check(lib.rf_dropout(ptr(x), ptr(y), dcode(x.dtype), float(p), int(seed), int(offset), x.numel(), stream()), "rf_dropout")
    return y


def dist_masked_attention(q, k, xyz, bins, att, B, L_, H, dq):
    _need_cuda(q, k, xyz, bins, att)
    check(lib.rf_dist_masked_attention(ptr(q), ptr(k), ptr(xyz), ptr(bins), ptr(att), dcode(att.dtype), B, L_, H, dq,
                                       stream()), "rf_dist_masked_attention")


def dist_masked_attention_bwd(q, k, xyz, bins, datt, B, L_, H, dq):
    """Backward of dist_masked_attention (rf_dist_masked_attention_bwd): q (scaled, as the forward saw it) and k contiguous fp32
    [B, L, H*dq], xyz contiguous fp32 [B, L, 3, 3], bins fp32 [H], datt contiguous fp32 [B, H, L, L] = the gradient of the
    probabilities.  Returns (d q, d k fp32 [B, L, H*dq], ds fp32 [B, H, L, L] = the logits' gradient, exactly 0 at a masked
    entry).  xyz has no gradient (the mask is piecewise constant)."""
    _need_cuda(q, k, xyz, bins, datt)
    HD = H * dq
    for t_ in (q, k):
        if t_.dtype != F32 or tuple(t_.shape) != (B, L_, HD) or not t_.is_contiguous():
            raise ValueError(f"dist_masked_attention_bwd: contiguous fp32 q and k [{B}, {L_}, {HD}]")
    if xyz.dtype != F32 or tuple(xyz.shape) != (B, L_, 3, 3) or not xyz.is_contiguous():
        raise ValueError(f"dist_masked_attention_bwd: contiguous fp32 xyz [{B}, {L_}, 3, 3]")
    if bins.dtype != F32 or bins.numel() != H or not bins.is_contiguous():
        raise ValueError(f"dist_masked_attention_bwd: contiguous fp32 bins [{H}]")
    if datt.dtype != F32 or tuple(datt.shape) != (B, H, L_, L_) or not datt.is_contiguous():
        raise ValueError(f"dist_masked_attention_bwd: contiguous fp32 datt [{B}, {H}, {L_}, {L_}]")
    d_q, d_k = (torch.empty(B, L_, HD, device=q.device, dtype=F32) for _ in range(2))
    ds = torch.empty(B, H, L_, L_, device=q.device, dtype=F32)
    check(lib.rf_dist_masked_attention_bwd(ptr(q), ptr(k), ptr(xyz), ptr(bins), ptr(datt), ptr(d_q), ptr(d_k), ptr(ds), B, L_, H,
                                           dq, stream()), "rf_dist_masked_attention_bwd")
    return d_q, d_k, ds


# --------------------------------------------------------------------------------------------- SE(3)
def knn_mask(xyz, aa_idx, k, kmin=9):
    B, L_ = xyz.shape[:2]
    mask = torch.empty(B, L_, L_, device=xyz.device, dtype=torch.uint8)
    _need_cuda(xyz, aa_idx)
    check(lib.rf_knn_mask(ptr(xyz), ptr(aa_idx), ptr(mask), B, L_, k, kmin, stream()), "rf_knn_mask")
    return mask


def edges_from_mask(mask, capacity, zero_tail=False):
    """count = [min(edges, capacity), edges]; src/dst beyond count[0] are never read by the consumers (zero_tail: zeroed
    instead of left uninitialised -- the functional dispatcher op returns fully defined tensors)."""
    B, L_, _ = mask.shape
    dev = mask.device
    _need_cuda(mask)
    mk = (lambda n: zeros(n, device=dev, dtype=torch.int32)) if zero_tail else (lambda n: torch.empty(n, device=dev, dtype=torch.int32))
    src = mk(capacity)
    dst = mk(capacity)
    eid = torch.empty(B, L_, L_, device=dev, dtype=torch.int32)
    count = torch.empty(2, device=dev, dtype=torch.int32)
    ws = torch.empty(2 * B * L_, device=dev, dtype=torch.int32)
    check(lib.rf_edges_from_mask(ptr(mask), ptr(src), ptr(dst), ptr(eid), ptr(count), ptr(ws), B, L_, capacity, stream()),
          "rf_edges_from_mask")
    return src, dst, eid, count


def se3_edge_geometry(xyz, edge_emb, src, dst, count, capacity):
    B, L_ = xyz.shape[:2]
    de = edge_emb.shape[-1]
    basis = torch.empty(capacity, 34, device=xyz.device, dtype=F32)
    feat = torch.empty(capacity, de + 1, device=xyz.device, dtype=F32)
    _need_cuda(xyz, edge_emb)
    check(lib.rf_se3_edge_geometry(ptr(xyz), ptr(edge_emb), ptr(src), ptr(dst), ptr(count), ptr(basis), ptr(feat),
                                   de + 1, L_, de, capacity, stream()), "rf_se3_edge_geometry")
    return basis, feat


def se3_message(R0, R1, basis, h0, h1, src, count, mo, dout, mi0, mi1, capacity):
    msg = torch.empty(capacity, mo, 2 * dout + 1, device=basis.device, dtype=F32)  # rows >= count are never read
    check(lib.rf_se3_message(ptr(R0), ptr(R1), ptr(basis), ptr(h0), ptr(h1), ptr(src), ptr(count), ptr(msg), mo, dout,
                             mi0, mi1, capacity, stream()), "rf_se3_message")
    return msg


def se3_radial_message_supported(mo, dout, mi0, mi1, ki):
    return bool(lib.rf_se3_radial_message_supported(int(mo), int(dout), int(mi0), int(mi1), int(ki)))


def se3_radial_message(feat, ki, net0, net1, basis, h0, h1, src, count, mo, dout, mi0, mi1, eps, capacity, zero_tail=False):
    """Fused radial MLP + message (csrc/se3.hip: rf_se3_radial_message): feat fp32 [capacity, ld] = [edge embedding | r];
    net_di = packed fp32 parameters of net (di, dout) (layout: include/rfmi.h).  Hidden vectors and radial outputs never exist."""
    _need_cuda(feat, net0, net1, basis, h0, h1, src, count)
    for t in (feat, net0, net1, h0, h1):
        if t is not None and t.dtype != F32:
            raise TypeError("se3_radial_message: fp32 operands")
    for t in (net0, net1, h0, h1):
        if t is not None and not t.is_contiguous():
            raise TypeError("se3_radial_message: contiguous operands")
    # rows >= count are never read (zero_tail: defined anyway, for the functional dispatcher op)
    msg = (zeros if zero_tail else torch.empty)(capacity, mo, 2 * dout + 1, device=basis.device, dtype=F32)
    check(lib.rf_se3_radial_message(ptr(feat), feat.stride(0), ki, ptr(net0), ptr(net1), ptr(basis), ptr(h0), ptr(h1), ptr(src),
                                    ptr(count), ptr(msg), mo, dout, mi0, mi1, float(eps), capacity, stream()),
          "rf_se3_radial_message")
    return msg


def se3_attention(k0, k1, q0, q1, v0, v1, eid, heads, mk0, mk1, mv0, mv1, V, L_, skip0=None, skip1=None):
    """out_d [V, mv_d (+ skip channels), 2d+1]: the attention result in the leading channels; with skip_d the node's
    input features are appended behind it (GCat, ea/modules.py:903-928) -- one buffer, no concatenation pass."""
    dev = k0.device
    c0 = mv0 + (skip0.shape[1] if skip0 is not None else 0)
    c1 = mv1 + (skip1.shape[1] if skip1 is not None else 0)
    out0 = torch.empty(V, c0, 1, device=dev, dtype=F32)
    out1 = torch.empty(V, c1, 3, device=dev, dtype=F32)
    _need_cuda(k0, q0, v0, eid)
    check(lib.rf_se3_attention(ptr(k0), ptr(k1), ptr(q0), ptr(q1), ptr(v0), ptr(v1), ptr(eid), ptr(out0), ptr(out1),
                               heads, mk0, mk1, mv0, mv1, V, L_, c0, 3 * c1, stream()), "rf_se3_attention")
    if skip0 is not None:
        copy(skip0, out0[:, mv0:])
    if skip1 is not None:
        copy(skip1, out1[:, mv1:])
    return out0, out1


def se3_norm_bias(v, bias, deg):
    V, m, _ = v.shape
    y = torch.empty_like(v)
    check(lib.rf_se3_norm_bias(ptr(v), ptr(bias), ptr(y), V, m, deg, stream()), "rf_se3_norm_bias")
    return y


def se3_gram(v, deg):
    V, m, _ = v.shape
    s = torch.empty(V, m * m, device=v.device, dtype=F32)
    check(lib.rf_se3_gram(ptr(v), ptr(s), V, m, deg, stream()), "rf_se3_gram")
    return s


def se3_attn_apply(att, x, m_out, deg):
    V, m_in, nc = x.shape
    y = torch.empty(V, m_out, nc, device=x.device, dtype=F32)
    check(lib.rf_se3_attn_apply(ptr(att), ptr(x), ptr(y), V, m_out, m_in, deg, stream()), "rf_se3_attn_apply")
    return y


# ---- backward of the SE(3) node layers and of the graph attention (csrc/se3.hip; fp32 in every compute mode)
def _f32c(name, t, shape):
    """t is a contiguous fp32 device tensor of `shape` (ValueError otherwise)"""
    if not torch.is_tensor(t) or t.dtype != F32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        got = f"{t.dtype} {tuple(t.shape)}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{name}: a contiguous fp32 tensor {list(shape)} is needed, got {got}")


def se3_attention_bwd(k0, k1, q0, q1, v0, v1, eid, g0, g1, heads, mk0, mk1, mv0, mv1, V, L_):
    """Backward of se3_attention (rf_se3_attention_bwd): k_d / v_d per edge [cap, m, 2d+1], q_d per node [V, m, 2d+1], eid the
    dense int32 map [B, L, L]; g_d fp32 [V, C_d, 2d+1] with C_d >= mv_d, the gradient of out_d -- the whole GCat buffer's gradient
    may be handed in, its leading mv_d channels are read.  Returns (dk0, dk1, dq0, dq1, dv0, dv1), shaped like k, q and v; edge rows
    at or above the edge count are not written (they are allocated, never read by a consumer)."""
    _need_cuda(k0, k1, q0, q1, v0, v1, eid, g0, g1)
    if L_ > 1024:
        raise ValueError(f"se3_attention_bwd: chain lengths up to 1024, got {L_}")
    if L_ <= 0 or V <= 0 or V % L_ or heads <= 0 or any(m % heads for m in (mk0, mk1, mv0, mv1)):
        raise ValueError(f"se3_attention_bwd: V = {V}, L = {L_}, heads = {heads}, channels {(mk0, mk1, mv0, mv1)}")
    cap = k0.shape[0]
    for name, t, m, d in (("k0", k0, mk0, 0), ("k1", k1, mk1, 1), ("v0", v0, mv0, 0), ("v1", v1, mv1, 1)):
        _f32c("se3_attention_bwd " + name, t, (cap, m, 2 * d + 1))
    _f32c("se3_attention_bwd q0", q0, (V, mk0, 1))
    _f32c("se3_attention_bwd q1", q1, (V, mk1, 3))
    if eid.dtype != torch.int32 or tuple(eid.shape) != (V // L_, L_, L_) or not eid.is_contiguous():
        raise ValueError(f"se3_attention_bwd: eid must be a contiguous int32 [{V // L_}, {L_}, {L_}] tensor")
    for name, t, m, d in (("g0", g0, mv0, 0), ("g1", g1, mv1, 1)):
        if t.dim() != 3 or t.shape[1] < m:
            raise ValueError(f"se3_attention_bwd {name}: [V, >= {m}, {2 * d + 1}] is needed, got {tuple(t.shape)}")
        _f32c("se3_attention_bwd " + name, t, (V, t.shape[1], 2 * d + 1))
    dk0, dk1, dq0, dq1, dv0, dv1 = (torch.empty_like(t) for t in (k0, k1, q0, q1, v0, v1))
    check(lib.rf_se3_attention_bwd(ptr(k0), ptr(k1), ptr(q0), ptr(q1), ptr(v0), ptr(v1), ptr(eid), ptr(g0), ptr(g1), g0.shape[1],
                                   3 * g1.shape[1], ptr(dk0), ptr(dk1), ptr(dq0), ptr(dq1), ptr(dv0), ptr(dv1), heads, mk0, mk1,
                                   mv0, mv1, V, L_, stream()), "rf_se3_attention_bwd")
    return dk0, dk1, dq0, dq1, dv0, dv1


def se3_norm_bias_bwd(v, bias, g, deg):
    """Backward of se3_norm_bias (rf_se3_norm_bias_bwd): v, g fp32 [V, m, 2 deg + 1], bias fp32 [m].  Returns (dv, dbias)."""
    _need_cuda(v, bias, g)
    if not torch.is_tensor(v) or v.dim() != 3 or v.shape[2] != 2 * deg + 1 or v.numel() == 0:
        raise ValueError(f"se3_norm_bias_bwd: v must be a non-empty [V, m, {2 * deg + 1}] tensor")
    V, m, _ = v.shape
    _f32c("se3_norm_bias_bwd v", v, v.shape)
    _f32c("se3_norm_bias_bwd g", g, v.shape)
    _f32c("se3_norm_bias_bwd bias", bias, (m,))
    ws_bytes = int(lib.rf_se3_norm_bias_bwd_ws_bytes(V, m, deg))
    ws = torch.empty(ws_bytes // 8, device=v.device, dtype=torch.float64)
    dv = torch.empty_like(v)
    dbias = torch.empty(m, device=v.device, dtype=F32)
    check(lib.rf_se3_norm_bias_bwd(ptr(v), ptr(bias), ptr(g), ptr(dv), ptr(dbias), V, m, deg, ptr(ws), ws_bytes, stream()),
          "rf_se3_norm_bias_bwd")
    return dv, dbias


def se3_gram_bwd(v, ds, deg, dv=None):
    """Backward of se3_gram (rf_se3_gram_bwd): v fp32 [V, m, 2 deg + 1], ds fp32 [V, m*m].  dv: a gradient of v to add to, in place
    (GAttentiveSelfInt's apply path); None: a fresh tensor.  Returns dv."""
    _need_cuda(v, ds, dv)
    if not torch.is_tensor(v) or v.dim() != 3 or deg not in (0, 1) or v.shape[2] != 2 * deg + 1 or v.numel() == 0:
        raise ValueError("se3_gram_bwd: v must be a non-empty [V, m, 2 deg + 1] tensor of degree 0 or 1")
    V, m, _ = v.shape
    _f32c("se3_gram_bwd v", v, v.shape)
    _f32c("se3_gram_bwd ds", ds, (V, m * m))
    acc = dv is not None
    if acc:
        _f32c("se3_gram_bwd dv", dv, v.shape)
    else:
        dv = torch.empty_like(v)
    check(lib.rf_se3_gram_bwd(ptr(v), ptr(ds), ptr(dv), int(acc), V, m, deg, stream()), "rf_se3_gram_bwd")
    return dv


def se3_attn_apply_bwd(att, x, g, m_out, deg):
    """Backward of se3_attn_apply (rf_se3_attn_apply_bwd): att fp32 [V, m_out*m_in], x fp32 [V, m_in, 2 deg + 1], g fp32
    [V, m_out, 2 deg + 1].  Returns (datt like att, dx like x)."""
    _need_cuda(att, x, g)
    if not torch.is_tensor(x) or x.dim() != 3 or deg not in (0, 1) or x.shape[2] != 2 * deg + 1 or x.numel() == 0 or m_out <= 0:
        raise ValueError("se3_attn_apply_bwd: x must be a non-empty [V, m_in, 2 deg + 1] tensor of degree 0 or 1")
    V, m_in, nc = x.shape
    if m_out * m_in > 8192:
        raise ValueError(f"se3_attn_apply_bwd: m_out * m_in = {m_out * m_in} is beyond the 8192 probabilities a block keeps")
    _f32c("se3_attn_apply_bwd x", x, x.shape)
    _f32c("se3_attn_apply_bwd att", att, (V, m_out * m_in))
    _f32c("se3_attn_apply_bwd g", g, (V, m_out, nc))
    datt, dx = torch.empty_like(att), torch.empty_like(x)
    check(lib.rf_se3_attn_apply_bwd(ptr(att), ptr(x), ptr(g), ptr(datt), ptr(dx), V, m_out, m_in, deg, stream()),
          "rf_se3_attn_apply_bwd")
    return datt, dx


def layernorm_act_bwd(x, g, gamma, beta, *, eps=1e-5, act=L.ACT_NONE):
    """Backward of layernorm(..., act=act) over the last dim at any width (rf_layernorm_act_bwd): x fp32 (the forward's input), g
    fp32 gradient of the activation's output, act = L.ACT_LEAKY or L.ACT_NONE.  Returns (dx, dgamma [D], dbeta [D]), fp32."""
    _need_cuda(x, g, gamma, beta)
    if act not in (L.ACT_NONE, L.ACT_LEAKY):
        raise ValueError("layernorm_act_bwd: act must be ACT_NONE or ACT_LEAKY")
    if not torch.is_tensor(x) or x.dim() < 1 or x.numel() == 0:
        raise ValueError("layernorm_act_bwd: x must be a non-empty tensor")
    D = x.shape[-1]
    rows = x.numel() // D
    _f32c("layernorm_act_bwd x", x, x.shape)
    _f32c("layernorm_act_bwd g", g, x.shape)
    _f32c("layernorm_act_bwd gamma", gamma, (D,))
    _f32c("layernorm_act_bwd beta", beta, (D,))
    if rows > 64 * 65535:
        raise ValueError(f"layernorm_act_bwd: at most {64 * 65535} rows, got {rows}")
    ws_bytes = int(lib.rf_layernorm_act_bwd_ws_bytes(rows, D))
    ws = torch.empty(ws_bytes // 8, device=x.device, dtype=torch.float64)
    dx = torch.empty_like(x)
    dgamma = torch.empty(D, device=x.device, dtype=F32)
    dbeta = torch.empty(D, device=x.device, dtype=F32)
    check(lib.rf_layernorm_act_bwd(ptr(x), ptr(g), ptr(gamma), ptr(beta), float(eps), int(act), ptr(dx), ptr(dgamma), ptr(dbeta),
                                   rows, D, ptr(ws), ws_bytes, stream()), "rf_layernorm_act_bwd")
    return dx, dgamma, dbeta


def coord_apply(xyz, disp):
    out = torch.empty_like(xyz)
    check(lib.rf_coord_apply(ptr(xyz), ptr(disp), ptr(out), xyz.shape[0] * xyz.shape[1], stream()), "rf_coord_apply")
    return out


def center_ca(xyz):
    y = torch.empty_like(xyz)
    check(lib.rf_center_ca(ptr(xyz), ptr(y), xyz.shape[0] * xyz.shape[1], stream()), "rf_center_ca")
    return y


def scale_rows(x, w, rows, D, out=None):
    """out[r, :] = x[r, :] * w[r]  (out defaults to a fresh tensor; pass out=x for in place)."""
    if out is None:
        out = torch.empty_like(x)
    _need_cuda(x, w, out)
    check(lib.rf_scale_rows(ptr(x), ptr(out), dcode(x.dtype), ptr(w), rows, D, stream()), "rf_scale_rows")
    return out


def fill(y, value=0.0):
    """y[...] = value through rf_fill (fp32 / bf16 contiguous tensors; int32 tensors are zero-filled as fp32 words)."""
    _need_cuda(y)
    if not y.is_contiguous():
        raise ValueError("fill: contiguous tensors only")
    if y.dtype == torch.int32:
        if value != 0:
            raise ValueError("fill: int32 tensors can only be zeroed")
        code = L.RF_F32
    else:
        code = dcode(y.dtype)
    check(lib.rf_fill(ptr(y), code, float(value), y.numel(), stream()), "rf_fill")
    return y


def zeros(*shape, device, dtype):
    return fill(torch.empty(*shape, device=device, dtype=dtype), 0.0)


def check_inputs(msa, seq, aa_idx, d_input, max_len):
    """One launch + one 12-byte read-back: (token out of range, aa_idx out of range, aa_idx not strictly increasing)."""
    ref = aa_idx if aa_idx is not None else (msa if msa is not None else seq)
    _need_cuda(msa, seq, aa_idx)
    flags = zeros(4, device=ref.device, dtype=torch.int32)
    L_ = aa_idx.shape[-1] if aa_idx is not None else 1
    check(lib.rf_check_inputs(ptr(msa), msa.numel() if msa is not None else 0, ptr(seq), seq.numel() if seq is not None else 0,
                              ptr(aa_idx), aa_idx.numel() if aa_idx is not None else 0, L_, d_input, max_len, ptr(flags),
                              stream()), "rf_check_inputs")
    f = flags.tolist()
    return bool(f[0]), bool(f[1]), bool(f[2])


def onehot(idx, n_classes, out=None, out_ld=None, col0=0, dtype=F32):
    rows = idx.numel()
    if out is None:
        out = torch.empty(*idx.shape, n_classes, device=idx.device, dtype=dtype)
        out_ld = n_classes
    _need_cuda(idx, out)
    check(lib.rf_onehot(ptr(idx), ptr(out), dcode(out.dtype), out_ld, col0, n_classes, rows, stream()), "rf_onehot")
    return out


def seqsep_feature(aa_idx, out, out_ld, col):
    B, L_ = aa_idx.shape
    _need_cuda(aa_idx, out)
    check(lib.rf_seqsep_feature(ptr(aa_idx), ptr(out), dcode(out.dtype), out_ld, col, B, L_, stream()), "rf_seqsep_feature")
    return out


def add_pos_enc(x, aa_idx, pe, two_d):
    B, N, L_, D = x.shape
    y = torch.empty_like(x)
    _need_cuda(x, aa_idx, pe)
    check(lib.rf_add_pos_enc(ptr(x), ptr(aa_idx), ptr(pe), ptr(y), B, N, L_, D, 1 if two_d else 0, stream()), "rf_add_pos_enc")
    return y


# Shortest sequence the model sends to the fused FAVOR+ kernel (the C ABI itself has no floor).  The kernel's smallest tile is
# 64 rows, so a short sequence is mostly padding; the floor is the smallest of {16, 32, 48, 64} at which the fused attend still
# beats the unfused chain.  Measured (tools/favor_bench.py --ragged, MI355X, bf16, pair layout B = 4, L x L x 288, 8 heads, q|k|v
# projection included, eager launches, rows / columns; profiles/r07_favor_ragged.json), fused vs unfused in us:
#   L = 16: 46 vs 151 / 46 vs 150     L = 32: 45 vs 151 / 45 vs 151     L = 48: 63 vs 201 / 63 vs 203     L = 64: 76 vs 320 / 76 vs 319
# The fused route wins 3.2-4.2x at every candidate (both are launch-bound there: 2 launches against a dozen), so speed alone puts
# the floor at 16.  It is 32 because of a test written for the other route: at 16 the bf16 full-model parity test
# (tests/test_modules_gpu.py::test_full_model_shapes_and_parity, L = 16, two-and-two blocks) came out at a distogram argmax
# agreement of 0.785 against its bound of 0.8 -- the fused kernel rounds q', k' and the context at other places than the chain
# that bound was set on, while its own error against the oracle at short lengths is that of the chain.  The existing
# module tests run at lengths 8 to 24; 32 is the smallest measured candidate above them.
FAVOR_FUSED_MIN_LS = 32


def favor_fused_applies(Ls, softmax, dh, m, dtype):
    """Python mirror of what rf_favor_attention accepts, plus the model's floor: 16-bit operands, dim_head 64, 266 features,
    any sequence length with the ReLU features, up to 256 rows with the softmax features (their key maximum spans the whole
    sequence, which must fit one tile)."""
    if not (is_h16(dtype) and dh == 64 and m == 266):
        return False
    if Ls < FAVOR_FUSED_MIN_LS:
        return False
    return Ls <= 256 or not softmax


def favor_attention(qkv, pc, out, x_strides, o_strides, q_off, k_off, v_off, n_b, n_o, n_h, seq_len, dim_head,
                    n_features, softmax_kernel, eps):
    _need_cuda(qkv, pc, out)
    if not (is_h16(qkv.dtype) and pc.dtype == qkv.dtype and out.dtype == qkv.dtype):
        raise TypeError("favor_attention is the 16-bit MFMA path (q|k|v, projection and output in the library's 16-bit type)")
    xs = L.I64x4(*[int(v) for v in x_strides])
    os_ = L.I64x3(*[int(v) for v in o_strides])
    check(lib.rf_favor_attention(ptr(qkv), ptr(pc), ptr(out), C.byref(xs), C.byref(os_), q_off, k_off, v_off, n_b, n_o,
                                 n_h, seq_len, dim_head, n_features, 1 if softmax_kernel else 0, eps, stream()),
          "rf_favor_attention")
    return out


# Fused residual + next-LayerNorm epilogue of the persistent GEMM (csrc/gemm_fast.hip, round 3: row-contiguous register image,
# one barrier per tile): the 288-wide pair rows (256 x 288 tiles) and the 384-wide MSA rows (128 x 384 tiles).  RF_NO_FUSED_LN=1
# restores the separate rf_layernorm launch for A/B timing.
FUSE_LN = not bool(int(__import__("os").environ.get("RF_NO_FUSED_LN", "0")))
# the generic tile kernel's fused form (any N <= 384 whose rows fit one tile; slower than GEMM + rf_layernorm on the forward's
# shapes, so opt-in: tests/test_kernels_gpu.py exercises it)
FUSE_LN_ANY = False


def ffn_pack(w1, w2, dtype=None):
    """Both feed-forward weight matrices (w1 [hidden, D], w2 [D, hidden], nn.Linear layout) in the fragment order
    rf_ffn_fused streams them (include/rfmi.h): per chunk of 32 hidden units D/16 one-KB pieces of W1, then D/16 of W2."""
    hid, D = w1.shape
    if w2.shape != (D, hid) or D % 32 or hid % 32:
        raise ValueError(f"ffn_pack: w1 {tuple(w1.shape)} / w2 {tuple(w2.shape)}")
    NC, KS, NT = hid // 32, D // 32, D // 16
    w1 = w1.detach().float().view(NC, 2, 16, KS, 4, 8).permute(0, 3, 1, 4, 2, 5)      # (c, ks, ht, fq, fr, j)
    w2 = w2.detach().float()
    NTH = NT // 2
    if NTH % 2 == 0:
        # paired column order of the kernel (csrc/ffn.hip: PAIRED): within a wave's half of the columns, MFMA tile i, row r holds
        # output column 32 (i >> 1) + 8 (r >> 2) + 4 (i & 1) + (r & 3) -- a lane's values of tiles 2 q, 2 q + 1 are 8 consecutive columns
        i = torch.arange(NTH).view(NTH, 1)
        r = torch.arange(16).view(1, 16)
        col = 32 * (i // 2) + 8 * (r // 4) + 4 * (i % 2) + (r % 4)                    # [NTH, 16]
        rows = torch.cat([half * NTH * 16 + col.reshape(-1) for half in range(2)]).to(w2.device)
        w2 = w2[rows]
    w2 = w2.view(NT, 16, NC, 2, 4, 4).permute(2, 0, 4, 1, 3, 5)      # (c, nt, fq, fr, j >> 2, j & 3)
    packed = torch.cat([w1.reshape(NC, -1), w2.reshape(NC, -1)], 1)
    return packed.to(dtype if dtype is not None else h16()).contiguous()


# One-launch feed-forward (csrc/ffn.hip).  At the forward's shapes it ties with the two-GEMM path on time (402 vs 397-417 us per MSA
# block, 511-525 vs 485-518 us per pair block; 315.8-317.0 vs 316.6-317.4 ms per forward on the same box) -- the weight stream of a
# 128-token tile through L2 -> LDS costs what the hidden round trip through HBM costs -- but it takes 0.15 TB of HBM traffic out of
# every forward (the hidden activations never exist in memory), so it is the default; RF_FUSED_FFN=0 restores the two GEMMs
# (DESIGN.md section 5 "fused feed-forward").
# RF_FUSED_FFN: 1 (default: both widths) | 0 (off) | 384 | 288 (only the feed-forward blocks of that model width)
_ffn_env = __import__("os").environ.get("RF_FUSED_FFN", "1").strip()
FUSE_FFN = _ffn_env not in ("", "0")
FUSE_FFN_WIDTHS = (int(_ffn_env),) if _ffn_env in ("288", "384") else (288, 384)


def ffn_fused_applies(xn, x_res, D, hidden):
    rows = x_res.numel() // D
    return (FUSE_FFN and is_h16(xn.dtype) and D in FUSE_FFN_WIDTHS and hidden % 32 == 0 and rows % 128 == 0 and rows >= 16384
            and x_res.is_contiguous() and xn.is_contiguous() and x_res.dtype == F32
            and 288 <= hidden and hidden * 4 <= 160 * 1024 - 153 * 1024 - 64)


def ffn_fused(xn, w_packed, b1, b2, x_res, next_ln=None):
    """x_res += W2 relu(W1 xn + b1) + b2 in one launch (csrc/ffn.hip); returns next_ln(x_res) in the 16-bit type when
    `next_ln` (an nn.LayerNorm) is given, else None."""
    D = x_res.shape[-1]
    rows = x_res.numel() // D
    hidden = b1.numel()
    _need_cuda(xn, w_packed, x_res)
    if w_packed.numel() != 2 * D * hidden or w_packed.dtype != xn.dtype:
        raise ValueError("ffn_fused: packed weights do not match (ops.ffn_pack)")
    out_ln = torch.empty(x_res.shape, device=x_res.device, dtype=xn.dtype) if next_ln is not None else None
    g = next_ln.weight.detach() if next_ln is not None else None
    b = next_ln.bias.detach() if next_ln is not None else None
    check(lib.rf_ffn_fused(ptr(xn), D, ptr(w_packed), ptr(b1), ptr(b2), ptr(x_res), D, ptr(x_res), D, ptr(out_ln), D, ptr(g), ptr(b),
                           float(next_ln.eps) if next_ln is not None else 0.0, rows, D, hidden, stream()), "rf_ffn_fused")
    return out_ln


def linear_residual_ln(x, w, bias, x_res, next_ln, xn_out=None):
    """x_res += x @ w^T + bias (fp32, in place).  If `next_ln` (an nn.LayerNorm) is given and the fused epilogue applies
    (bf16 operands, full rows per tile), also returns LayerNorm_next(x_res) in bf16 (written into `xn_out` when given: the
    row-panel callers pass a slice of one full-size tensor); otherwise returns None and the caller normalises with
    rf_layernorm."""
    N = w.shape[0]
    rows = x_res.numel() // N
    # whole rows per tile: the persistent GEMM normalises the updated rows in its epilogue (csrc/gemm_fast.hip)
    fused = (FUSE_LN and N in (288, 384) and rows % 256 == 0 and rows >= 16384) or (FUSE_LN_ANY and N <= 384 and N % 4 == 0)
    if fused and next_ln is not None and is_h16(x.dtype) and x_res.is_contiguous() and x.is_contiguous():
        xn = torch.empty(x_res.shape, device=x_res.device, dtype=x.dtype) if xn_out is None else xn_out
        linear(x, w, bias, out=x_res, residual=x_res,
               ln=(xn, next_ln.weight.detach(), next_ln.bias.detach(), next_ln.eps))
        return xn
    linear(x, w, bias, out=x_res, residual=x_res)
    return None
