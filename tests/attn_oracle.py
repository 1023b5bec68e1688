"""Float64 oracle of the two hand-scheduled attention files, csrc/favor.hip (fused FAVOR+) and csrc/tied.hip (tied MSA-row
attention and the collapsed position weights), shared by tests/test_attn_oracle_cpu.py and tests/test_attn_bound_gpu.py.  A plain
helper module, the sibling of tests/rowops_oracle.py and tests/gemm_oracle.py; storage, comparison and the exponential
allowances are imported from rowops_oracle, not copied.

Forms.  Every form is written from the C ABI comment in include/rfmi.h and takes what the library takes: 1-D storage tensors,
element offsets of the pointers, the stride arrays, lengths, att_ld, eps, qscale.  Addressing is done with index tensors built
from those numbers alone.  16-bit operands are taken as they are stored, so the reference is exact on what the kernel saw.
Every form takes `dtype`:
  float64   the reference: the documented formula, no intermediate rounding.
  float32   together with h16 = the build's 16-bit type: the STAGED evaluation, the yardstick.  The same formula in float32
            (torch's own exp / exp2, its own summation order), rounded to h16 exactly where the kernels' design puts a 16-bit
            operand, and nowhere else:
              FAVOR+  k' = phi(k Pc^T)                      favor.hip:317-320 (4-wave), 781-784 (8-wave): A operand of ctx += k' v
                      ctx = k'^T [v | 1], its ones column   favor.hip:336-337, 807-808: published to LDS as the A operand of
                        (d = 64) holding sum_s k'           num += ctx^T q'.  fp16 build: after the factor 2^-ceil(log2 seq_len)
                                                            applied to the fp32 sums (FV_CS, favor.hip:49-58; p.ctx_scale is set
                                                            from the true length at the end of rf_favor_attention)
                      q' = phi(q Pc^T)                      favor.hip:452-455, 931-934: B operand of num += ctx^T q'
                      out = num[:64] / num[64]              favor.hip:473-474, 952-953: the stored result
              tied    q * (w * qscale) when w != NULL       tied.hip:157 (one-pass), 340 (contraction-split): "the same rounding
                                                            point as q*w (rf.py:252)"; w * qscale is one fp32 product
                      att                                   tied.hip:201-202 (one-pass), 392-393 (split softmax): stored
                      out = att . v                         tied.hip:697-698: stored
              rf_poswise_collapsed has no 16-bit stage: 16-bit operands as stored, fp32 accumulators, fp32 w.
            Everything else is float32.

Bound.  Each of l2 / row / elem, exactly as rowops_oracle.compare defines them, is held to
    FACTOR * (the same error of the staged evaluation) + (the same functional of `extra`),        FACTOR = 8
(the kernels sum in another order and contract FMAs).  `extra` holds the analytic terms below.  They are computed from float64
values only, never from the kernel's output.

  exp2_allowance(t) -- the softmax feature map of the fused FAVOR+ kernel is exp2(t) + eps with t = x Pc^T - diag - max in fp32,
      Pc already carrying log2(e).  Of the (|t| + 2) 2^-23 of rowops_oracle.exp_allowance (the __expf = exp2(t log2 e) form) the two
      |t| 2^-24 terms are the rounding of the product t * log2(e) and the error of the constant log2(e): here neither exists (the
      product happened in pc, which the reference takes as stored).  What is left of them is the last rounding of the fp32
      argument itself, |t| 2^-24 in the exponent, i.e. ln(2) |t| 2^-24 = (ln 2 / 2) |t| 2^-23 relative in the result.  The hardware
      exp2 is good to 1 ulp (2^-23) and the addition of eps rounds once more: ((ln 2 / 2) |t| + 2) 2^-23 exp2(t) per feature,
      never more than exp_allowance(t ln 2) (checked in the CPU test).
      Through the ratio (favor_extra): out_i = sum_s a_is v_s with a_is = (q'_i . k'_s) / sum_s' (q'_i . k'_s'), every weight
      positive.  Absolute feature errors dq'_im, dk'_sm move the unnormalised weight W_is = q'_i . k'_s by at most
      E_is = sum_m (dq'_im k'_sm + q'_im dk'_sm), a relative error d_s = E_is / W_is of key weight a_is, which moves out by at most
      sum_s a_is d_s |v_s| (numerator) + |out_i| sum_s a_is d_s (denominator) = ((E |v|)_i + |out_i| sum_s E_is) / sum_s W_is.
      The ReLU feature map has no exponential: its extra is zero.
  softmax_allowance(t) -- rowops_oracle's, on the stabilised float64 logits, for att (tied) and w (position weights): both
      kernels use __expf.
  accumulation of a long fp32 contraction -- the tied logits sum K = 32 N products of 16-bit values in fp32 (K up to 8192), the
      position weights K = D.  The staged evaluation's own error there is ONE sample of summation noise, not a ceiling, so the
      per-element accumulation term of tests/gemm_oracle.py is added: |delta logit_ij| <= op_term_h16(K) * sum |q~||k|,
      op_term_h16(K) = (K + 8) 2^-23, with q~ the (scaled) query.  softmax_carry() takes a logit perturbation delta through the
      softmax the way softmax_allowance takes its own: y_j (delta_j + sum_l y_l delta_l).
      The FAVOR+ context (K = seq_len <= 700 here) and attention . V (K = L <= 256) do NOT get this term: their fp32 sums feed a
      16-bit rounding (2^-9 / 2^-12 relative against K 2^-24 <= 4e-5), the measured ratios (profiles/r11_attention_bound.json)
      stay below 1 without it, and the reordered-staging condition of the CPU test holds without it.

Nothing else is fixed in advance.  test_attn_oracle_cpu.py checks, without a GPU, the forms against naive loops, that a staged
evaluation summed in another order stays inside the bound (the bound does not reject a correct kernel) and that six planted
value faults leave it (it does reject a wrong one).

The constants mirror include/rfmi.h and the kernels' dispatch, so the module imports without the library."""
import math

import torch

from rowops_oracle import (FACTOR, PAD, RECORDS, assert_untouched, compare, exp_allowance, image_storage,  # noqa: F401
                           out_storage, randn, rnd, softmax_allowance, strided_offsets, tied_sym, f32)
from gemm_oracle import op_term_h16

F64, F32 = torch.float64, torch.float32
FV_DH, FV_M, FV_MPAD = 64, 266, 288
LOG2E = 1.4426950408889634
ATTN_RECORDS = []  # the records of this module's comparisons (rowops_oracle.RECORDS also holds the row-op tests' own)

# ------------------------------------------------------------------------------------------------ route codes (rfmi.h)
ROUTES = {}
for _w8 in (0, 1):
    for _i, _ls in enumerate((64, 128, 256)):
        for _sm in (0, 1):
            for _tail in (0, 1):
                if not (_w8 and _sm and _ls == 256):  # the 8-wave softmax kernel ends at the 128-row tile
                    ROUTES[100 + 12 * _w8 + 4 * _i + 2 * _sm + _tail] = "favor%d_%d_%s%s" % (
                        8 if _w8 else 4, _ls, "softmax" if _sm else "relu", "_tail" if _tail else "")
for _i in range(4):
    for _sc in (0, 1):
        for _tail in (0, 1):
            ROUTES[200 + 4 * _i + 2 * _sc + _tail] = "logits_%d%s%s" % (64 * (_i + 1), "_scale" if _sc else "", "_tail" if _tail else "")
    for _tail in (0, 1):
        ROUTES[240 + 2 * _i + _tail] = "av_%d%s" % (64 * (_i + 1), "_tail" if _tail else "")
ROUTES.update({220: "split_nkb1", 221: "split_nkb1_scale", 222: "split_nkb2", 224: "split_nkb3", 226: "split_nkb4"})
for _nt in (1, 2, 3, 4, 5, 6, 7, 8, 12, 16):
    ROUTES[260 + _nt] = "poswise_nt%d" % _nt


def favor_code(seq_len, softmax_kernel, four_wave=False):
    """the instantiation rf_favor_attention picks (favor.hip, launch_favor)"""
    ls = 64 if seq_len <= 64 else 128 if seq_len <= 128 else 256
    nchunks = (seq_len + 255) // 256 if seq_len > 256 else 1
    w4 = four_wave or (softmax_kernel and ls == 256)
    return 100 + (0 if w4 else 12) + 4 * (64, 128, 256).index(ls) + 2 * int(bool(softmax_kernel)) + int(seq_len != nchunks * ls)


def tile_of(L):
    return (L + 63) // 64 * 64


def logits_code(L, att_ld, scale):
    return 200 + 4 * (tile_of(L) // 64 - 1) + 2 * int(bool(scale)) + int(L != tile_of(L) or att_ld != L)


def split_code(L, scale):
    return 220 + 2 * (L // 256 - 1) + int(bool(scale))


def split_applies(L, N, ws_elems, B, H):
    """tied.hip, tied_logits_split: the contraction-split route runs iff this holds (dense att, workspace given)"""
    if L % 256 or L > 1024 or N % 2:
        return False
    nsplit = 2 if L == 256 else 1
    while N // nsplit > 64 and N % (nsplit * 2) == 0:
        nsplit *= 2
    nper = N // nsplit
    return not (nper > 64 or nper < 4 or nper & 1 or ws_elems < B * H * L * L * nsplit)


def av_code(L, att_ld):
    return 240 + 2 * (tile_of(L) // 64 - 1) + int(L != tile_of(L) or att_ld != L)


def poswise_code(N):
    return 260 + N // 16


# ------------------------------------------------------------------------------------------------ allowances
def exp2_allowance(t):
    """absolute error allowance of exp2(t) + eps for a float64 exponent t (derivation in the module docstring)"""
    return (0.5 * math.log(2.0) * t.abs() + 2) * 2.0 ** -23 * torch.exp2(t)


def softmax_carry(y, delta):
    """what a perturbation |delta_j| of the logits does to y = softmax(logits) over the last dim"""
    return y * (delta + (y * delta).sum(-1, keepdim=True))


def _stage(x, h16):
    """round a float32 tensor to the build's 16-bit type where the kernel forms a 16-bit operand; float64 passes"""
    return x if h16 is None or x.dtype == F64 else x.to(h16).to(x.dtype)


def _check_dtype(dtype, h16):
    assert (dtype == F64 and h16 is None) or (dtype == F32 and h16 in (torch.bfloat16, torch.float16)), (dtype, h16)


def both(form, h16, *a, **kw):
    """(float64 reference, staged evaluation in the build whose 16-bit type is h16), both as float64 tensors"""
    r64 = form(*a, dtype=F64, **kw)
    st = form(*a, dtype=F32, h16=h16, **kw)
    if isinstance(r64, tuple):
        return r64[0], st[0].to(F64), r64[1:]
    return r64, st.to(F64), ()


# ------------------------------------------------------------------------------------------------ FAVOR+
def favor_rows(qkv, base, x_strides, col_off, n_b, n_o, n_h, seq_len):
    """[n_b, n_o, n_h, seq_len, 64]: the row of (b, o, s) of head h starts at b xs[0] + o xs[1] + s xs[2] + h xs[3]"""
    off = strided_offsets(base + col_off, (x_strides[0], x_strides[1], x_strides[3], x_strides[2], 1),
                          (n_b, n_o, n_h, seq_len, FV_DH), qkv.device)
    return qkv[off]


def favor_out_offsets(o_strides, n_b, n_o, n_h, seq_len, device="cpu"):
    """[n_b, n_o, n_h, seq_len, 64] element offsets from the out pointer: b os[0] + o os[1] + s os[2] + h * 64 + d"""
    return strided_offsets(0, (o_strides[0], o_strides[1], FV_DH, o_strides[2], 1), (n_b, n_o, n_h, seq_len, FV_DH), device)


def favor_features(x, P, softmax_kernel, eps, is_query):
    """phi(x Pc^T) in x's dtype, and the exponent t (softmax features) or None"""
    a = x @ P.transpose(-1, -2)
    if not softmax_kernel:
        return a.clamp_min(0) + eps, None
    # |x|^2 d^-1/2 log2(e) / 2 with d = 64 (the kernel's fp32 constant 0.0625f * 1.4426950408889634f)
    c = 0.0625 * LOG2E if x.dtype == F64 else f32(f32(0.0625) * f32(LOG2E))
    diag = (x * x).sum(-1, keepdim=True) * c
    mx = a.amax(-1, keepdim=True) if is_query else a.amax((-1, -2), keepdim=True)
    t = a - (diag + mx)
    return torch.exp2(t) + eps, t


def favor_combine(qp, kp, v, h16, seq_chunk=None):
    """out [.., Sq, 64] = (q' (k'^T v)) / (q' . sum_s k') from features qp [.., Sq, M], kp [.., S, M] and values v [.., S, 64].
    Staged (h16 given, float32): the context with its ones column is rounded to h16, in the fp16 build after the factor
    2^-ceil(log2 S) on the fp32 sums.  seq_chunk = c: the context is accumulated over the sequence in REVERSED chunks of c rows
    (another summation order of the same staging)."""
    S = kp.shape[-2]
    v1 = torch.cat([v, torch.ones_like(v[..., :1])], -1)
    if seq_chunk is None:
        ctx = kp.transpose(-1, -2) @ v1
    else:
        ctx = torch.zeros(kp.shape[:-2] + (kp.shape[-1], FV_DH + 1), dtype=kp.dtype, device=kp.device)
        for s0 in reversed(range(0, S, seq_chunk)):
            ctx = ctx + kp[..., s0:s0 + seq_chunk, :].transpose(-1, -2) @ v1[..., s0:s0 + seq_chunk, :]
    if h16 == torch.float16:
        ctx = ctx * 2.0 ** -math.ceil(math.log2(S))
    ctx = _stage(ctx, h16)
    num = qp @ ctx
    return num[..., :FV_DH] / num[..., FV_DH:]


def favor_attention(qkv, pc, x_strides, o_strides, q_off, k_off, v_off, n_b, n_o, n_h, seq_len, softmax_kernel, eps, *,
                    base=PAD, dtype, h16=None, seq_chunk=None, detail=False):
    """rf_favor_attention (dim_head 64, 266 features).  qkv: 1-D storage, `base` the element offset of the qkv pointer; pc: the
    [288, 64] projection as stored (rows >= 266 are not features).  Returns (out [n_b, n_o, n_h, seq_len, 64], element offsets
    of those values from the out pointer); with detail=True a dict of the intermediates as third member.  Rows >= seq_len take
    part in nothing: they are never addressed."""
    _check_dtype(dtype, h16)
    e = f32(eps)
    q, k, v = (favor_rows(qkv, base, x_strides, c, n_b, n_o, n_h, seq_len).to(dtype) for c in (q_off, k_off, v_off))
    P = pc.reshape(FV_MPAD, FV_DH)[:FV_M].to(dtype)
    qp, tq = favor_features(q, P, softmax_kernel, e, True)
    kp, tk = favor_features(k, P, softmax_kernel, e, False)
    qp, kp = _stage(qp, h16), _stage(kp, h16)
    out = _stage(favor_combine(qp, kp, v, h16, seq_chunk), h16)
    off = favor_out_offsets(o_strides, n_b, n_o, n_h, seq_len, qkv.device)
    if detail:
        return out, off, dict(qp=qp, kp=kp, tq=tq, tk=tk, v=v)
    return out, off


def favor_extra(out64, d):
    """the exp2 allowance carried through the ratio (module docstring); d: the float64 detail of favor_attention"""
    if d["tq"] is None:
        return None
    dq, dk = exp2_allowance(d["tq"]), exp2_allowance(d["tk"])
    E = dq @ d["kp"].transpose(-1, -2) + d["qp"] @ dk.transpose(-1, -2)
    den = (d["qp"] @ d["kp"].transpose(-1, -2)).sum(-1, keepdim=True)
    return (E @ d["v"].abs() + out64.abs() * E.sum(-1, keepdim=True)) / den


# ------------------------------------------------------------------------------------------------ tied attention
def qk_offsets(base, strides, B, N, H, L, device="cpu"):
    """[B, N, H, L, 32]: element (b, n, h, l, d) at base + b s[0] + n s[1] + h s[2] + l s[3] + d (q, k, v and out)"""
    return strided_offsets(base, tuple(strides) + (1,), (B, N, H, L, 32), device)


def att_offsets(base, B, H, L, att_ld, device="cpu"):
    """[B, H, L, L]: element (b, h, i, j) at ((b H + h) L + i) att_ld + j"""
    return strided_offsets(base, (H * L * att_ld, L * att_ld, att_ld, 1), (B, H, L, L), device)


def att_pad_offsets(base, B, H, L, att_ld, device="cpu"):
    """the columns [L, att_ld) of every row, or None when att is dense"""
    return strided_offsets(base + L, (att_ld, 1), (B * H * L, att_ld - L), device) if att_ld > L else None


def sym_offsets(base, B, H, L, sym_ld, device="cpu"):
    return strided_offsets(base, (L * L * sym_ld, L * sym_ld, sym_ld, 1), (B, L, L, H), device)


def scaled_queries(q, q_off, qk_strides, w, w_off, w_strides, qscale, B, H, N, L, *, dtype, h16=None):
    """[B, N, H, L, 32]: q (w qscale) when w is given (rounded to h16 in the staged evaluation), q as stored otherwise"""
    qv = q[qk_offsets(q_off, qk_strides, B, N, H, L, q.device)].to(dtype)
    if w is None:
        return qv
    wv = w[strided_offsets(w_off, tuple(w_strides) + (1,), (B, H, N, L), w.device)].to(dtype) * f32(qscale)
    return _stage(qv * wv.permute(0, 2, 1, 3)[..., None], h16)


def tied_logits(q, k, qk_strides, w, w_strides, qscale, B, H, N, L, att_ld, *, q_off=PAD, k_off=PAD, w_off=PAD, dtype,
                h16=None, n_halves=False, detail=False):
    """rf_tied_logits_ld: att [B, H, L, L] = softmax_j sum_{n,d} (w[b,h,n,i] qscale) q[b,n,h,i,d] k[b,n,h,j,d] (staged: as it is
    stored).  att_ld only places the values (att_offsets / att_pad_offsets); the symmetrised map comes from the STORED att
    through tied_sym.  n_halves: the MSA rows are summed in two halves that are added at the end, as the contraction-split
    kernel does."""
    _check_dtype(dtype, h16)
    assert att_ld >= L
    qv = scaled_queries(q, q_off, qk_strides, w, w_off, w_strides, qscale, B, H, N, L, dtype=dtype, h16=h16)
    kv = k[qk_offsets(k_off, qk_strides, B, N, H, L, k.device)].to(dtype)

    def part(n0, n1):
        return torch.einsum("bnhid,bnhjd->bhij", qv[:, n0:n1], kv[:, n0:n1])
    lg = part(0, N // 2) + part(N // 2, N) if n_halves and N > 1 else part(0, N)
    t = lg - lg.amax(-1, keepdim=True)
    att = _stage(torch.softmax(t, -1), h16)
    if detail:
        return att, dict(t=t, logits=lg, part=part, mag=torch.einsum("bnhid,bnhjd->bhij", qv.abs(), kv.abs()))
    return att


def tied_logits_extra(d, N):
    """__expf in the softmax + the fp32 accumulation of K = 32 N products, carried through the softmax; d: float64 detail"""
    return softmax_allowance(d["t"]) + softmax_carry(torch.softmax(d["t"], -1), op_term_h16(32 * N) * d["mag"])


def tied_av(att, att_ld, v, v_strides, o_strides, B, H, N, L, *, att_off=PAD, v_off=PAD, dtype, h16=None):
    """rf_tied_av_ld: out[b,n,h,i,:] = sum_j att[b,h,i,j] v[b,n,h,j,:] from the stored att (columns >= L are not summed: the
    library relies on their being zeros).  Returns (out [B, N, H, L, 32], element offsets from the out pointer)."""
    _check_dtype(dtype, h16)
    a = att[att_offsets(att_off, B, H, L, att_ld, att.device)].to(dtype)
    vv = v[qk_offsets(v_off, v_strides, B, N, H, L, v.device)].to(dtype)
    out = _stage(torch.einsum("bhij,bnhjd->bnhid", a, vv), h16)
    return out, qk_offsets(0, o_strides, B, N, H, L, att.device)


def poswise_collapsed(xn, u, B, N, L, D, H, scale, *, xn_off=PAD, u_off=PAD, dtype, h16=None, detail=False):
    """rf_poswise_collapsed: softmax over n of scale * sum_c xn[b,n,l,c] u[b,l,h,c], returned as [B, H, L, N] (the softmax row
    last; the library stores w[b,h,n,l]: poswise_offsets).  No 16-bit stage: h16 is accepted and unused."""
    x = xn[strided_offsets(xn_off, (N * L * D, L * D, D, 1), (B, N, L, D), xn.device)].to(dtype)
    uu = u[strided_offsets(u_off, (L * H * D, H * D, D, 1), (B, L, H, D), u.device)].to(dtype)
    t = torch.einsum("bnlc,blhc->bhln", x, uu) * f32(scale)
    t = t - t.amax(-1, keepdim=True)
    w = torch.softmax(t, -1)
    if detail:
        return w, dict(t=t, mag=torch.einsum("bnlc,blhc->bhln", x.abs(), uu.abs()) * abs(f32(scale)))
    return w


def poswise_offsets(base, B, H, N, L, device="cpu"):
    """[B, H, L, N] offsets of w[b,h,n,l] in the dense [B, H, N, L] result"""
    return strided_offsets(base, (H * N * L, N * L, 1, L), (B, H, L, N), device)


def poswise_extra(d, D):
    return softmax_allowance(d["t"]) + softmax_carry(torch.softmax(d["t"], -1), op_term_h16(D) * d["mag"])


# ------------------------------------------------------------------------------------------------ inputs
def projection(seed, log2e, h16, device="cpu"):
    """pc [288, 64] as PerformerSelfAttention.proj_scaled builds it: a seeded orthogonal-block Gaussian (performer-pytorch's
    construction), times dim_head^-1/4, times log2(e) for the softmax features, zero rows from 266 on, in the build's type"""
    g = torch.Generator().manual_seed(seed)
    blocks = []
    for i in range(-(-FV_M // FV_DH)):
        qm, _ = torch.linalg.qr(torch.randn(FV_DH, FV_DH, generator=g), mode="reduced")
        blocks.append(qm.t()[:min(FV_DH, FV_M - i * FV_DH)])
    p = torch.randn(FV_M, FV_DH, generator=g).norm(dim=1)[:, None] * torch.cat(blocks) * FV_DH ** -0.25
    if log2e:
        p = p * LOG2E
    pp = torch.zeros(FV_MPAD, FV_DH)
    pp[:FV_M] = p
    return pp.to(h16).to(device)


# ------------------------------------------------------------------------------------------------ comparison
def check(name, got, ref64, staged, extra=None, *, route=None, build=None, exact=False, check=True):
    """rowops_oracle.compare (the three metrics and the bound are its own) + one `[attn]` line + this module's record"""
    rec = compare(name, got, ref64, staged, extra, exact=exact, route=ROUTES.get(route, route), check=False)
    rec["build"] = build
    ATTN_RECORDS.append(rec)
    print("[attn] %s route=%s build=%s " % (name, rec["route"], build) + " ".join(
        "%s %.3e staged %.3e extra %.3e ratio %.3f" % (m, rec[m]["err"], rec[m]["e32"], rec[m]["extra"], rec[m]["ratio"])
        for m in ("l2", "row", "elem")))
    rec["ok"] = all(rec[m]["ratio"] <= 1.0 for m in ("l2", "row", "elem"))
    if check:
        assert rec["ok"], (name, rec)
    return rec


# ------------------------------------------------------------------------------------------------ test inputs
def favor_case(layout, n_b, n_o, n_h, S, *, qk_std=1.0, v_mean=0.0, seed=0, h16, device="cpu", gap=2):
    """q | k | v of n_b * n_o * n_h items of S rows in NaN-padded storage.  layout: "contiguous" / "strided" are the two layouts
    of tests/test_favor_ragged_gpu._layout (sequence rows contiguous; sequences strided along the other axis) with rows of
    3 * 64 n_h + 16 elements and q | k | v from column 8 on; "headmajor": [n_b, n_o, 3 n_h, S + gap, 64] tiles
    (x_strides[3] = (S + gap) * 64).  Every sequence is followed by `gap` rows that exist in the storage and hold NaN."""
    inner, n = FV_DH * n_h, S + gap
    if layout == "headmajor":
        xs, cols = (n_o * 3 * n_h * n * 64, 3 * n_h * n * 64, 64, n * 64), (0, n_h * n * 64, 2 * n_h * n * 64)
        os_ = (n_o * n * inner, n * inner, inner)
    else:
        W = 3 * inner + 16
        cols = (8, 8 + inner, 8 + 2 * inner)
        if layout == "strided":
            xs, os_ = (n * n_o * W, W, n_o * W, 64), (n * n_o * inner, inner, n_o * inner)
        else:
            assert layout == "contiguous"
            xs, os_ = (n_o * n * W, n * W, W, 64), (n_o * n * inner, n * inner, inner)
    dims = (n_b, n_o, n_h, S, FV_DH)
    vals = randn((3,) + dims, seed, device)
    vals[:2] *= qk_std
    vals[2] += v_mean
    off = torch.stack([strided_offsets(PAD + c, (xs[0], xs[1], xs[3], xs[2], 1), dims, device) for c in cols])
    assert off.unique().numel() == off.numel()
    return dict(qkv=image_storage(off, vals, h16, extra=4096), xs=xs, os=os_, cols=cols, dims=dims,
                args=(xs, os_) + cols + (n_b, n_o, n_h, S))


def tied_case(B, H, N, L, *, with_w, spread, seed=0, h16, device="cpu", rowmajor=False, gap=3):
    """q, k, v (NaN-padded 16-bit storages, head-major [B, N, H, L + gap, 32] or row-major [B, N, L, H * 32]) and, with_w, the
    position weights w [B, H, N, 4 ceil(L / 4)] (softmax over n of a Gaussian, fp32, NaN in the row pad) with qscale = 32^-0.5.
    spread: the width of a row of logits, about 5 standard deviations; q is scaled to give it."""
    Lp = L + gap
    st = (N * L * H * 32, L * H * 32, 32, H * 32) if rowmajor else (N * H * Lp * 32, H * Lp * 32, Lp * 32, 32)
    off = qk_offsets(PAD, st, B, N, H, L, device)
    qscale = 32 ** -0.5
    sigma = spread / 5.0
    c = dict(st=st, qscale=qscale, w=None, ws=None, Lw=0)
    if with_w:
        Lw = (L + 3) // 4 * 4
        wv = torch.softmax(randn((B, H, N, L), seed + 3, device), 2)
        c.update(w=image_storage(strided_offsets(PAD, (H * N * Lw, N * Lw, Lw, 1), (B, H, N, L), device), wv, F32),
                 ws=(H * N * Lw, N * Lw, Lw), Lw=Lw)
        qstd = sigma / (qscale * math.sqrt(32 * math.e / N))
    else:
        qstd = sigma / math.sqrt(32 * N)
    c["q"] = image_storage(off, qstd * randn((B, N, H, L, 32), seed, device), h16)
    c["k"] = image_storage(off, randn((B, N, H, L, 32), seed + 1, device), h16)
    c["v"] = image_storage(off, randn((B, N, H, L, 32), seed + 2, device), h16)
    return c


# ------------------------------------------------------------------------------------------------ planted value faults
PLANTED = ("block16_scaled_1.02", "key_dropped_last_row", "padded_key_phi0_eps", "logit_past_len_zero", "value_columns_swapped",
           "split_range_added_twice")


def planted_faults(h16):
    """Six wrong kernels, imitated on the staged evaluation in Python (CPU): {name: the bound rejects it}.  The FAVOR+ faults are
    planted where each matters most: the softmax features with wide logits, where most features sit at eps."""
    res = {}

    def rejected(name, bad, r64, staged, extra=None):
        res[name] = not check("planted/" + name, bad, r64, staged, extra, build=str(h16), check=False)["ok"]
        ATTN_RECORDS.pop()

    S, eps = 40, 1e-4
    c = favor_case("contiguous", 1, 2, 3, S, qk_std=2.0, seed=5, h16=h16)
    pc = projection(1, True, h16)
    r64, _, d64 = favor_attention(c["qkv"], pc, *c["args"], True, eps, dtype=F64, detail=True)
    st, _, d = favor_attention(c["qkv"], pc, *c["args"], True, eps, dtype=F32, h16=h16, detail=True)
    extra = favor_extra(r64, d64)
    bad = st.clone()
    bad[0, 1, 2, 16:32] *= 1.02
    rejected(PLANTED[0], _stage(bad, h16), r64, st, extra)
    bad = st.clone()
    kp = d["kp"].clone()
    kp[..., 7, :] = 0
    bad[..., S - 1, :] = _stage(favor_combine(d["qp"][..., S - 1:, :], kp, d["v"], h16), h16)[..., 0, :]
    rejected(PLANTED[1], bad, r64, st, extra)
    kp = torch.cat([d["kp"], torch.full_like(d["kp"][..., :1, :], f32(eps))], -2)  # the clamped copy of the last row enters
    bad = _stage(favor_combine(d["qp"], kp, torch.cat([d["v"], d["v"][..., -1:, :]], -2), h16), h16)
    rejected(PLANTED[2], bad, r64, st, extra)

    B, H, N, L = 1, 2, 8, 40
    t = tied_case(B, H, N, L, with_w=False, spread=4.0, seed=9, h16=h16)
    a = (t["q"], t["k"], t["st"], None, None, t["qscale"], B, H, N, L, L)
    a64, d64 = tied_logits(*a, dtype=F64, detail=True)
    ast, d = tied_logits(*a, dtype=F32, h16=h16, detail=True)
    extra = tied_logits_extra(d64, N)
    lg = torch.cat([d["logits"], torch.zeros_like(d["logits"][..., :1])], -1)  # key L: 0 instead of -inf
    bad = ast.clone()
    bad[0, 1, 3] = _stage(torch.softmax(lg[0, 1, 3], -1), h16)[:L]
    rejected(PLANTED[3], bad, a64, ast, extra)
    lg = d["logits"] + d["part"](0, 4)
    rejected(PLANTED[5], _stage(torch.softmax(lg, -1), h16), a64, ast, extra)
    att = image_storage(att_offsets(PAD, B, H, L, L), a64, h16)
    o64, _ = tied_av(att, L, t["v"], t["st"], t["st"], B, H, N, L, dtype=F64)
    ost, _ = tied_av(att, L, t["v"], t["st"], t["st"], B, H, N, L, dtype=F32, h16=h16)
    bad = ost.clone()
    bad[0, 5, 1, :, 3], bad[0, 5, 1, :, 4] = ost[0, 5, 1, :, 4], ost[0, 5, 1, :, 3]
    rejected(PLANTED[4], bad, o64, ost)
    return res
