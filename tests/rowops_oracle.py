"""Float64 oracle of the row kernels of csrc/ops.hip (norms, softmaxes, element-wise), shared by the row-op tests.  A plain
helper module, the sibling of tests/gemm_oracle.py.

Forms.  Every op is written from its C ABI comment in include/rfmi.h and takes what the library takes: 1-D storage tensors,
pointer offsets (elements), leading dimensions / strides, groups, act, eps.  Addressing is done with index tensors built from
those numbers alone, so a stride mistake in a test shows as a mismatch instead of being mirrored.  Every form takes `dtype`:
float64 is the reference, float32 is the plain single-precision evaluation of the same formula (two-pass statistics, torch's
own exp); `both(form, out_dtype, ...)` returns the float64 result and the float32 one rounded to the output dtype.  16-bit
inputs are taken as they are stored, so the reference is exact on what the kernel saw.

Storage.  `image_storage` holds values on the image of the op's addressing and NaN everywhere else (gap columns between D and
the leading dimension, rows past `rows`, PAD elements before and after): a stray read poisons the result.  `out_storage` is a
sentinel everywhere; `assert_untouched` compares bit patterns outside the documented image (and, where the header documents a
zero pad, asserts exact zeros there).

Bound.  compare() computes three errors of `got` against the float64 reference over every element,
    l2    ||got - ref|| / ||ref||
    row   max_r ||got_r - ref_r|| / rms_r ||ref_r||                     (as tests/test_se3_kernels_gpu.py)
    elem  max_i |got_i - ref_i| / max(|ref_i|, rms of ref over i's row)  (one wrong element of a wide row cannot hide)
and holds each to  FACTOR * kappa * (the same error of the rounded float32 evaluation) + (the same functional of `extra`).
FACTOR = 8 as in test_se3_kernels_gpu.py: the kernels sum in another order, use rsqrtf and contract FMAs.  Nothing else is
fixed in advance; the two analytic terms, both computed from float64 values and never from the kernel's output:

  exp_allowance(t): the kernels use __expf(t) = exp2(t * log2(e)).  The product t * log2(e) is rounded once (relative 2^-24),
      which moves the exponent by |t| log2(e) 2^-24 in absolute terms, i.e. the result by |t| log2(e) ln(2) 2^-24 = |t| 2^-24
      relative; the hardware exp2 is good to 1 ulp (2^-23) and the constant log2(e) carries its own 2^-24 relative error,
      another |t| 2^-24.  Together (|t| + 1) 2^-23 relative; with one more ulp for the rounding of the result:
      (|t| + 2) 2^-23 |exp(t)| per element.  softmax_allowance() carries it through the normalisation: element c of a row has
      relative error d_c = (|t_c| + 2) 2^-23 in its numerator and at most sum_j y_j d_j in the denominator.
  kappa (InstanceNorm only): the kernels take the variance in one pass, E[x^2] - E[x]^2.  A relative perturbation u of either
      moment changes the difference by u (E[x^2] + E[x]^2) / var <= 2 u (1 + mean^2 / var), against u for the two-pass form, so
      the bound is multiplied by kappa = max over (b, c) of 1 + mean^2 / var, from the float64 statistics.  LayerNorm is
      two-pass in registers and gets none.

  sums_bound(): each fp64 sum of rf_instnorm_stats is a float64 sum of fp32 block partials.  A partial is a chain of at most P
      fp32 additions (P = 128 pixels in the generic kernel; at most 512 / ppi + ppi <= 512 in the vectorised one), one rounding
      each (the squares enter through fmaf): |partial - exact| <= P 2^-24 sum |terms|.  The float64 additions across blocks add
      2^-53 per step, below that by 2^-29.  So |sums - exact| <= P 2^-24 * sum |x| (resp. sum x^2) per (b, c).

The constants mirror include/rfmi.h so that the module imports without the library (tests/test_rowops_oracle_cpu.py checks
the forms against naive loops on a machine without a GPU; test_cabi pins the header)."""
import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_ELU, ACT_LEAKY = 0, 1, 2, 4
PAD = 64
SENTINEL = -1234.0
FACTOR = 8.0
F64 = torch.float64

# route codes of rf_rowops_last_route (include/rfmi.h)
ROUTES = {
    1: "ln_rows8_288", 2: "ln_rows8_384", 3: "sym_rows8_288", 4: "sym_rows8_384", 5: "ln_vec2", 6: "ln_vec4", 7: "ln_vec_h16",
    8: "ln_narrow8", 9: "ln_narrow16",
    10: "ln_generic1", 11: "ln_generic2", 12: "ln_generic5", 13: "ln_generic6", 14: "ln_generic8", 15: "ln_generic16",
    16: "ln_generic36",
    20: "sym_generic1", 21: "sym_generic2", 22: "sym_generic5", 23: "sym_generic6", 24: "sym_generic8", 25: "sym_generic16",
    26: "sym_generic36",
    30: "in_stats_generic", 31: "in_stats_vec", 32: "in_apply_generic", 33: "in_apply_vec_fixed", 34: "in_apply_vec_modulo",
    40: "axpby_scalar", 41: "axpby_vec", 42: "tile_scalar", 43: "tile_vec",
}


def generic_code(D, sym=False):
    """the instantiation launch_ln picks for the generic kernel"""
    return (20 if sym else 10) + sum(D > t for t in (64, 128, 320, 384, 512, 1024))


def f32(v):
    """a Python float as the library receives it (a C float argument)"""
    return torch.tensor(v, dtype=torch.float32).item()


def ar(n, device):
    return torch.arange(n, device=device, dtype=torch.int64)


def rnd(x, dtype):
    """round to dtype, back in float64"""
    return x.to(dtype).to(F64)


def both(form, out_dtype, *a, **kw):
    """(float64 reference, float32 evaluation rounded to out_dtype), both as float64 tensors"""
    return form(*a, dtype=F64, **kw), rnd(form(*a, dtype=torch.float32, **kw), out_dtype)


# ------------------------------------------------------------------------------------------------ storage
def randn(shape, seed, device="cpu"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=F64).to(device)


def image_storage(off, values, dtype, extra=0):
    """1-D storage: values (any shape matching off) at the offsets `off` (from the start of the storage, all >= PAD), NaN at
    every other element, PAD + extra elements of NaN behind the last one"""
    off = off.reshape(-1)
    assert off.min().item() >= PAD, "keep PAD elements in front of the pointer"
    st = torch.full((off.max().item() + 1 + PAD + extra,), float("nan"), dtype=dtype, device=off.device)
    st[off] = values.reshape(-1).to(dtype)
    return st


def out_storage(off, dtype, extra=0, sentinel=SENTINEL):
    off = off.reshape(-1)
    assert off.min().item() >= PAD
    assert off.unique().numel() == off.numel(), "the output layout maps two elements to one offset"
    return torch.full((off.max().item() + 1 + PAD + extra,), sentinel, dtype=dtype, device=off.device)


def outside_image(st, off):
    m = torch.ones(st.numel(), dtype=torch.bool, device=st.device)
    m[off.reshape(-1)] = False
    return m


def assert_untouched(before, after, off, zero_off=None, what=None):
    """every element of the output storage outside `off` (and outside zero_off, which must hold exact zeros) keeps its
    sentinel bit for bit"""
    assert before.shape == after.shape and before.dtype == after.dtype
    it = {8: torch.int64, 4: torch.int32, 2: torch.int16}[before.element_size()]
    out = outside_image(after, off)
    if zero_off is not None:
        z = after.reshape(-1)[zero_off.reshape(-1)]
        assert (z.view(it) == 0).all(), (what, "the documented zero pad is not exactly +0")
        out[zero_off.reshape(-1)] = False
    bad = out & (after.reshape(-1).view(it) != before.to(after.device).reshape(-1).view(it))
    assert not bad.any(), (what, f"{int(bad.sum())} elements outside the image were written, first at offset {int(bad.nonzero()[0])}")


# ------------------------------------------------------------------------------------------------ offsets
def row_offsets(base, ld, rows, D, device="cpu"):
    """[rows, D]: base + r * ld + c"""
    return base + ar(rows, device)[:, None] * ld + ar(D, device)[None, :]


def strided_offsets(base, strides, dims, device="cpu"):
    """[*dims]: base + sum_k i_k * strides[k]"""
    off = torch.full((), base, dtype=torch.int64, device=device)
    for k, (s, n) in enumerate(zip(strides, dims)):
        shape = [1] * len(dims)
        shape[k] = n
        off = off + (ar(n, device) * s).reshape(shape)
    return off


# ------------------------------------------------------------------------------------------------ forms
def _act(y, act):
    if act == ACT_RELU:
        return y.clamp_min(0)
    if act == ACT_LEAKY:
        return torch.where(y > 0, y, 0.01 * y)
    if act == ACT_ELU:
        return torch.where(y > 0, y, torch.expm1(y.clamp_max(0)))
    assert act == ACT_NONE
    return y


def _ln(x, eps):
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    return d / torch.sqrt((d * d).mean(-1, keepdim=True) + f32(eps))


def layernorm(xs, x_off, x_ld, rows, D, gamma, beta, eps, groups=1, act=ACT_NONE, *, dtype):
    """rf_layernorm: [rows, D]; gamma / beta 1-D tensors of groups * D floats or None; row r uses group r % groups"""
    dev = xs.device
    y = _ln(xs[row_offsets(x_off, x_ld, rows, D, dev)].to(dtype), eps)
    if gamma is not None:
        gi = (ar(rows, dev)[:, None] % groups if groups > 1 else 0) * D + ar(D, dev)[None, :]
        gi = gi.expand(rows, D)
        y = y * gamma[gi].to(dtype) + beta[gi].to(dtype)
    return _act(y, act)


def sym_layernorm(ps, p_off, B, L, D, eps, *, dtype):
    """rf_sym_layernorm: [B*L*L, D], row (b, i, j) = LayerNorm(0.5 * (pair[b,i,j] + pair[b,j,i])) without affine"""
    dev = ps.device
    b, i, j, c = ar(B, dev)[:, None, None, None], ar(L, dev)[None, :, None, None], ar(L, dev)[None, None, :, None], ar(D, dev)
    a = ps[p_off + ((b * L + i) * L + j) * D + c].to(dtype)
    t = ps[p_off + ((b * L + j) * L + i) * D + c].to(dtype)
    return _ln(0.5 * (a + t), eps).reshape(B * L * L, D)


def instnorm_stats(xs, x_off, B, HW, C):
    """float64 (sums [B, C, 2] = (sum, sum of squares) over the HW pixels, abs [B, C, 2] = (sum |x|, sum x^2)) of NHWC x"""
    x = xs[strided_offsets(x_off, (HW * C, C, 1), (B, HW, C), xs.device)].to(F64)
    s, q = x.sum(1), (x * x).sum(1)
    return torch.stack([s, q], -1), torch.stack([x.abs().sum(1), q], -1)


def sums_bound(absum, P):
    return P * 2.0 ** -24 * absum


def instnorm_kappa(xs, x_off, B, HW, C):
    x = xs[strided_offsets(x_off, (HW * C, C, 1), (B, HW, C), xs.device)].to(F64)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    return (1 + mean * mean / var).max().item()


def instnorm(xs, x_off, B, HW, C, gamma, beta, eps, residual=None, act=ACT_NONE, *, dtype):
    """rf_instnorm_stats + rf_instnorm_apply: [B, HW, C]; gamma is None: centre only (x - mean).  Two-pass statistics (the
    biased variance of InstanceNorm2d).  residual: fp32 tensor [B, HW, C] or None."""
    x = xs[strided_offsets(x_off, (HW * C, C, 1), (B, HW, C), xs.device)].to(dtype)
    mean = x.mean(1, keepdim=True)
    d = x - mean
    if gamma is None:
        y = d
    else:
        y = d / torch.sqrt((d * d).mean(1, keepdim=True) + f32(eps)) * gamma.to(dtype) + beta.to(dtype)
    if residual is not None:
        y = y + residual.to(dtype)
    return _act(y, act)


def elu_allowance(y64):
    """the fast exponential in the ELU branch (y64: float64 value before the activation)"""
    return torch.where(y64 > 0, torch.zeros_like(y64), exp_allowance(y64.clamp_max(0)))


def exp_allowance(t):
    return (t.abs() + 2) * 2.0 ** -23 * torch.exp(t)


def softmax_allowance(t):
    """t: float64 stabilised logits (scale * x - row max) with the softmax over the last dim"""
    y = torch.softmax(t, -1)
    d = torch.where(torch.isfinite(t), (t.abs() + 2) * 2.0 ** -23, torch.zeros_like(t))
    return y * (d + (y * d).sum(-1, keepdim=True))


def softmax_logits(xs, x_off, x_bs, x_rs, x_cs, rows, cols, scale, nbatch=1, *, dtype):
    """[nbatch, rows, cols]: scale * x[z * x_bs + r * x_rs + c * x_cs] minus the row maximum"""
    t = xs[strided_offsets(x_off, (x_bs, x_rs, x_cs), (nbatch, rows, cols), xs.device)].to(dtype) * f32(scale)
    return t - t.max(-1, keepdim=True).values


def softmax(xs, x_off, x_bs, x_rs, x_cs, rows, cols, scale, nbatch=1, *, dtype):
    """rf_softmax (nbatch = 1, x_bs = 0) / rf_softmax_batched: [nbatch, rows, cols]"""
    return torch.softmax(softmax_logits(xs, x_off, x_bs, x_rs, x_cs, rows, cols, scale, nbatch, dtype=dtype), -1)


def tied_sym(att, *, dtype=F64):
    """the symmetrised map of rf_tied_softmax from the STORED att [B, H, L, L] -> [B, L, L, H]"""
    a = att.to(dtype)
    return (0.5 * (a + a.transpose(-1, -2))).permute(0, 2, 3, 1)


def poswise_logits(q0s, q0_off, q0_ld, ks, k_off, k_ld, k_col0, k_hs, dlen, B, N, L, H, scale, *, dtype):
    """[B, L, H, N]: scale * sum_c q0[b, l, h, c] k[b, n, l, h, c], minus the maximum over n"""
    dev = q0s.device
    qo = strided_offsets(q0_off, (L * q0_ld, q0_ld, dlen, 1), (B, L, H, dlen), dev)
    ko = strided_offsets(k_off + k_col0, (N * L * k_ld, L * k_ld, k_ld, k_hs, 1), (B, N, L, H, dlen), dev)
    q, k = q0s[qo].to(dtype), ks[ko].to(dtype)
    t = (q[:, None] * k).sum(-1).permute(0, 2, 3, 1) * f32(scale)
    return t - t.max(-1, keepdim=True).values


def poswise(*a, dtype):
    """rf_poswise: w [B, N, H, L] = softmax over n"""
    return torch.softmax(poswise_logits(*a, dtype=dtype), -1).permute(0, 3, 2, 1)


def poswise_qscale(qs_vals, w, qscale, *, dtype):
    """the in-place scaling: qs_vals [B, N, L, H, qs_dh] (as stored before the call) * w[b, n, h, l] * qscale"""
    return qs_vals.to(dtype) * (w.to(dtype).permute(0, 1, 3, 2)[..., None] * f32(qscale))


def weighted_msa_sum(xs, x_off, ws, w_off, B, N, L, D, *, dtype):
    """rf_weighted_msa_sum: [B, L, D] = sum_n w[(b * N + n) * L + l] * x[b, n, l, :]"""
    dev = xs.device
    x = xs[strided_offsets(x_off, (N * L * D, L * D, D, 1), (B, N, L, D), dev)].to(dtype)
    w = ws[strided_offsets(w_off, (N * L, L, 1), (B, N, L), dev)].to(dtype)
    return (w[..., None] * x).sum(1)


def favor_offsets(base, S, n, m_pad, transposed, device="cpu"):
    """[S, n, m_pad] offsets of feature f of row r of item S in the stored layout"""
    return strided_offsets(base, (n * m_pad, 1, n) if transposed else (n * m_pad, m_pad, 1), (S, n, m_pad), device)


def favor_exponent(ds, d_off, xs, x_off, xstr, n1, n2, S, n, m, m_pad, dh, is_query, transposed, *, dtype):
    dev = ds.device
    dash = ds[favor_offsets(d_off, S, n, m_pad, transposed, dev)[..., :m]].to(dtype)
    s = ar(S, dev)
    xb = (s // (n2 * n1)) * xstr[0] + ((s // n2) % n1) * xstr[1] + (s % n2) * xstr[2]
    x = xs[x_off + xb[:, None, None] + ar(n, dev)[None, :, None] * xstr[3] + ar(dh, dev)].to(dtype)
    diag = 0.5 * (x * x).sum(-1, keepdim=True) * float(dh) ** -0.5
    mx = dash.amax(-1, keepdim=True) if is_query else dash.amax((-1, -2), keepdim=True)
    return dash - diag - mx


def favor_features(*a, eps, dtype):
    """rf_favor_softmax_features: [S, n, m_pad] with exact zeros at features >= m (a[9] = m, a[10] = m_pad)"""
    t = favor_exponent(*a, dtype=dtype)
    m, m_pad = a[9], a[10]
    y = float(m) ** -0.5 * (torch.exp(t) + f32(eps))
    return F.pad(y, (0, m_pad - m))


def linattn_normalize(ns, n_off, num_ld, rows, dh, *, dtype):
    v = ns[row_offsets(n_off, num_ld, rows, dh + 1, ns.device)].to(dtype)
    return v[:, :dh] / v[:, dh:]


def axpby(x, a, z, b, *, dtype):
    y = f32(a) * x.to(dtype)
    return y if z is None else y + f32(b) * z.to(dtype)


def scale_rows(x, w, *, dtype):
    return x.to(dtype) * w.to(dtype)[:, None]


def tile_1d_feats(m1, B, L, P2):
    """[B, L, L, 2 * P2] float64: msa1d[b, i, :] | msa1d[b, j, :]"""
    v = m1.reshape(B, L, P2).to(F64)
    return torch.cat([v[:, :, None, :].expand(B, L, L, P2), v[:, None, :, :].expand(B, L, L, P2)], -1)


# ------------------------------------------------------------------------------------------------ comparison
RECORDS = []


def _metrics(err, ref):
    """(l2, row, elem) of an error tensor [R, W] against the reference [R, W]"""
    rn = ref.norm(dim=1)
    rms_rows = (rn * rn).mean().sqrt().clamp_min(1e-300)
    row_rms = (rn / ref.shape[1] ** 0.5)[:, None]
    den = torch.maximum(ref.abs(), row_rms).clamp_min(1e-300)
    return ((err.norm() / ref.norm().clamp_min(1e-300)).item(), (err.norm(dim=1).max() / rms_rows).item(), (err.abs() / den).max().item())


def compare(name, got, ref64, ref32, extra=None, *, kappa=1.0, exact=False, route=None, check=True):
    """got / ref64 / ref32 / extra: tensors of one shape whose last dim is the row.  Returns the record it printed.
    exact=True: the op is a copy or a conversion, got must equal ref32 (the float64 value rounded once) bit for bit."""
    ref = ref64.to(F64).reshape(-1, ref64.shape[-1])
    assert torch.isfinite(ref).all(), (name, "the reference is not finite: the test's own addressing reads a gap")
    g = got.to(F64).reshape(ref.shape).to(ref.device)
    r32 = ref32.to(F64).reshape(ref.shape)
    assert torch.isfinite(g).all(), (name, f"{int((~torch.isfinite(g)).sum())} non-finite results: a stray read")
    k = _metrics(g - ref, ref)
    e = _metrics(r32 - ref, ref)
    x = _metrics(extra.to(F64).reshape(ref.shape), ref) if extra is not None else (0.0, 0.0, 0.0)
    rec = dict(case=name, route=route, kappa=kappa, exact=exact)
    ok = True
    for nm, kk, ee, xx in zip(("l2", "row", "elem"), k, e, x):
        bound = FACTOR * kappa * ee + xx
        rec[nm] = dict(err=kk, e32=ee, extra=xx, ratio=kk / bound if bound > 0 else (0.0 if kk == 0 else float("inf")),
                       ratio_e32=kk / ee if ee > 0 else None)
        ok = ok and kk <= bound
    print("[rowops] %s route=%s kappa=%.3g " % (name, route, kappa) +
          " ".join("%s %.3e e32 %.3e ratio %.3f" % (nm, rec[nm]["err"], rec[nm]["e32"], rec[nm]["ratio"]) for nm in ("l2", "row", "elem")))
    RECORDS.append(rec)
    if exact:
        assert torch.equal(g, r32), (name, "not the float64 value rounded once", int((g != r32).sum()))
    else:
        assert min(e) > 0, (name, "the float32 evaluation is exact here: declare the comparison exact")
    if check:
        assert ok, (name, rec)
    return rec
