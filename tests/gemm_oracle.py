"""Descriptor-level float64 oracle of rf_gemm (include/rfmi.h), shared by the GEMM tests.  A plain helper module.

A test describes one rf_gemm call as a dict whose keys are the fields of rf_gemm_desc (`desc(...)` fills in the defaults) plus
the three pointer offsets a_off / b_off / c_off (elements from the start of the storage tensor to the pointer the library
gets).  Everything else follows from that dict alone:

  effective_operands(d, A_storage, B_storage)   float64 A[z, m, k], B[z, n, k]: the header's offset formulas evaluated literally
                                                with index tensors (batch decode, a_rc / a_ro / a_ri, kc / a_ko, conv im2col
                                                with zero padding and dilation);
  c_offsets(d)                                  element offset of every C(z, m, n) from the C pointer;
  make_operand / make_c / make_residual
                                                storage tensors whose every element OUTSIDE the image of those formulas is NaN
                                                (operands, residual: a stray read poisons the result) or a sentinel (C: a stray
                                                write is seen bit for bit), with 64 such elements before and after;
  check_bound(...)                              the per-element bound  |got - x| <= tol,
      tol = op_term * (mag + |bias| if the bias is folded into the accumulator) + 2^-22 (|x| + |prod|) + out |x| + tiny
                                                with prod = alpha A B^T, mag = |alpha| |A| |B|^T, x = the float64 result after bias,
                                                activation and residual.  op_term is the caller's (the kernel family's operand /
                                                accumulation precision); ELU adds 4e-6 |x| (the fast exponential).

The constants mirror include/rfmi.h, so the module imports without the library (tests/test_gemm_oracle_cpu.py checks the
formulas against naive loops on a machine without a GPU; test_cabi pins the header's values)."""
import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_ELU, ACT_RELU_EPS = 0, 1, 2, 3
BIAS_NONE, BIAS_COL, BIAS_ROW = 0, 1, 2
AMODE_PLAIN, AMODE_CONV3X3 = 0, 1
PAD = 64  # elements of NaN / sentinel before and after every storage

OUT_ROUND = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
OUT_TINY = {torch.float32: 1e-30, torch.bfloat16: 1e-30, torch.float16: 2.0 ** -24}  # fp16 subnormal spacing


def op_term_h16(K):
    """fp32 accumulation of exact 16-bit products (twice the textbook K 2^-24: the MFMA's summation order is undocumented)
    plus the generic kernel's fold of bias / alpha into the accumulator"""
    return (K + 8) * 2.0 ** -23


def op_term_f32(K):
    return (K + 4) * 2.0 ** -24


def op_term_split(K):
    """RF_F32X3 (include/rfmi.h): the dropped lo.lo product and the rounding of lo on either side, plus the accumulation"""
    return 3 * 2.0 ** -16 + K * 2.0 ** -23


def desc(M, N, K, **kw):
    d = dict(M=M, N=N, K=K, nb0=1, nb1=1, nb2=1, kc=0, a_mode=AMODE_PLAIN, a_rc=0, b_rc=0, c_rc=0, c_cc=0,
             a_bs=(0, 0, 0), a_ro=0, a_ri=K, a_ko=0, b_bs=(0, 0, 0), b_ro=0, b_ri=K, b_ko=0,
             c_bs=(0, 0, 0), c_ro=0, c_ri=N, c_co=0, conv_n=0, conv_h=0, conv_w=0, conv_c=0, conv_dil=0,
             a_off=PAD, b_off=PAD, c_off=PAD)
    unknown = set(kw) - set(d)
    assert not unknown, unknown
    d.update(kw)
    if d["a_mode"] == AMODE_CONV3X3:  # rf_gemm: kc = conv_c, weights [N][tap][c] with K contiguous
        assert K == 9 * d["conv_c"] and M == d["conv_n"] * d["conv_h"] * d["conv_w"]
        d["kc"], d["b_ko"] = d["conv_c"], d["conv_c"]
    elif d["kc"] <= 0:
        d["kc"] = K
    return d


def _split(idx, rc, ro, ri):
    return (idx // rc) * ro + (idx % rc) * ri if rc > 0 else idx * ri


def _batch(d, device):
    """z -> (z0, z1, z2) as in the header: z = (z0 * nb1 + z1) * nb2 + z2"""
    z = torch.arange(d["nb0"] * d["nb1"] * d["nb2"], device=device)
    z2 = z % d["nb2"]
    t = z // d["nb2"]
    return t // d["nb1"], t % d["nb1"], z2


def _zoff(d, bs, device):
    z0, z1, z2 = _batch(d, device)
    return z0 * bs[0] + z1 * bs[1] + z2 * bs[2]


def operand_offsets(d, side, device="cpu"):
    """(offsets [Z, R, K] from the operand pointer, valid [Z, R, K]): valid is False for a conv tap outside the picture"""
    K, kc = d["K"], d["kc"]
    k = torch.arange(K, device=device)
    if side == "a" and d["a_mode"] == AMODE_CONV3X3:
        h, w, c, dil = d["conv_h"], d["conv_w"], d["conv_c"], d["conv_dil"]
        m = torch.arange(d["M"], device=device)[:, None]
        tap, ch = (k // c)[None, :], (k % c)[None, :]
        pix = m % (h * w)
        ii = pix // w + (tap // 3 - 1) * dil
        jj = pix % w + (tap % 3 - 1) * dil
        valid = (ii >= 0) & (ii < h) & (jj >= 0) & (jj < w)
        off = ((m // (h * w)) * (h * w) + ii * w + jj) * c + ch
        Z = d["nb0"] * d["nb1"] * d["nb2"]
        return off[None].expand(Z, -1, -1), valid[None].expand(Z, -1, -1)  # the a_* strides are ignored
    R = d["M"] if side == "a" else d["N"]
    r = torch.arange(R, device=device)
    row = _split(r, d[side + "_rc"], d[side + "_ro"], d[side + "_ri"])
    off = _zoff(d, d[side + "_bs"], device)[:, None, None] + row[None, :, None] + ((k // kc) * d[side + "_ko"] + k % kc)[None, None, :]
    return off, torch.ones_like(off, dtype=torch.bool)


def c_offsets(d, device="cpu"):
    """element offset of C(z, m, n) from the C pointer, [Z, M, N]"""
    m, n = torch.arange(d["M"], device=device), torch.arange(d["N"], device=device)
    return (_zoff(d, d["c_bs"], device)[:, None, None] + _split(m, d["c_rc"], d["c_ro"], d["c_ri"])[None, :, None] +
            _split(n, d["c_cc"], d["c_co"], 1)[None, None, :])


def effective_operands(d, A_storage, B_storage):
    """float64 A[z, m, k], B[z, n, k] as the kernel is to see them (zero for a conv tap outside the picture)"""
    out = []
    for side, st in (("a", A_storage), ("b", B_storage)):
        off, valid = operand_offsets(d, side, st.device)
        off = off + d[side + "_off"]
        flat = st.reshape(-1)
        v = flat[torch.where(valid, off, torch.zeros_like(off))].double()
        out.append(torch.where(valid, v, torch.zeros_like(v)))
    return out


def _rand(n, seed, device="cpu"):
    return torch.randn(n, generator=torch.Generator(device=device).manual_seed(seed), dtype=torch.float64, device=device).float()


def _image_storage(off, base, dtype, seed, extra=0):
    """random values (rounded to dtype) on the image of `off` (+ base), NaN everywhere else, PAD elements of NaN behind"""
    device = off.device
    assert off.min().item() + base >= PAD
    size = base + off.max().item() + 1 + PAD + extra
    st = _rand(size, seed, device).to(dtype)
    keep = torch.zeros(size, dtype=torch.bool, device=device)
    keep[(off + base).reshape(-1)] = True
    st[~keep] = float("nan")
    return st


def make_operand(d, side, dtype, seed, device="cpu"):
    """1-D storage of operand `side` ('a' / 'b'): NaN in every gap (between row groups, between K chunks, columns [K, ri), the
    PAD elements before the first and after the last element the formulas reach)"""
    off, valid = operand_offsets(d, side, device)
    return _image_storage(off[valid], d[side + "_off"], dtype, seed)


def make_c(d, dtype, sentinel=-1234.0, extra=0, device="cpu"):
    """C storage filled with the sentinel (also the gap rows / columns of split layouts and the columns [N, c_ri))"""
    off = c_offsets(d, device)
    assert off.min().item() + d["c_off"] >= PAD
    assert off.reshape(-1).unique().numel() == off.numel(), "C layout maps two elements to one offset"
    return torch.full((d["c_off"] + off.max().item() + 1 + PAD + extra,), sentinel, dtype=dtype, device=device)


def make_residual(d, seed, res_off=None, device="cpu"):
    """fp32 residual in C's layout (pointer at res_off, default c_off): NaN outside the image"""
    return _image_storage(c_offsets(d, device), d["c_off"] if res_off is None else res_off, torch.float32, seed)


def gather_c(d, storage, off_base=None):
    off = c_offsets(d, storage.device) + (d["c_off"] if off_base is None else off_base)
    return storage.reshape(-1)[off]


def assert_untouched(d, before, after):
    """every element of the C storage outside the image of c_offsets holds its sentinel bit for bit"""
    assert before.shape == after.shape and before.dtype == after.dtype
    it = {4: torch.int32, 2: torch.int16}[before.element_size()]
    outside = torch.ones(before.numel(), dtype=torch.bool, device=after.device)
    outside[(c_offsets(d, after.device) + d["c_off"]).reshape(-1)] = False
    b, a = before.to(after.device).reshape(-1).view(it), after.reshape(-1).view(it)
    bad = outside & (a != b)
    assert not bad.any(), f"{int(bad.sum())} elements outside C were written, first at storage offset {int(bad.nonzero()[0])}"


def gemm_kwargs(d):
    """keyword arguments of ops.gemm for the descriptor"""
    kw = dict(batch=(d["nb0"], d["nb1"], d["nb2"]), a_off=d["a_off"], b_off=d["b_off"], c_off=d["c_off"],
              a_bs=d["a_bs"], a_row=(d["a_rc"], d["a_ro"], d["a_ri"]), a_ko=d["a_ko"],
              b_bs=d["b_bs"], b_row=(d["b_rc"], d["b_ro"], d["b_ri"]), b_ko=d["b_ko"], kc=d["kc"],
              c_bs=d["c_bs"], c_row=(d["c_rc"], d["c_ro"], d["c_ri"]), c_col=(d["c_cc"], d["c_co"]))
    if d["a_mode"] == AMODE_CONV3X3:
        kw["conv"] = (d["conv_n"], d["conv_h"], d["conv_w"], d["conv_c"], d["conv_dil"])
        kw["kc"] = 0
    return kw


def act_ref(x, act, nvalid, eps, mrow, ncol):
    if act == ACT_RELU:
        return x.clamp_min(0)
    if act == ACT_ELU:
        return F.elu(x)
    if act == ACT_RELU_EPS:
        valid = (mrow < -nvalid) if nvalid < 0 else (ncol < nvalid)
        return torch.where(valid, x.clamp_min(0) + eps, torch.zeros_like(x))
    return x


def reference(Ae, Be, *, alpha=1.0, bias=None, bias_mode=None, res=None, act=ACT_NONE, nvalid=0, eps=0.0, scale=None):
    """(x, prod, mag, |bias| broadcast) in float64 on the operands' device; scale [.., M, N]: the row-group scale of
    rf_gemm_desc.rs, applied to the biased product before the activation"""
    Ad, Bd = Ae.double(), Be.double()
    prod = alpha * (Ad @ Bd.transpose(-1, -2))
    mag = abs(alpha) * (Ad.abs() @ Bd.abs().transpose(-1, -2))
    M, N = prod.shape[-2:]
    x = prod
    babs = torch.zeros_like(prod)
    if bias is not None:
        b = bias.double().to(prod.device)
        bb = b[None, :] if bias_mode in (None, BIAS_COL) else b[:, None]
        x = x + bb
        babs = bb.abs().expand_as(prod)
    if scale is not None:
        s = scale.double().to(prod.device)
        x, prod, mag, babs = x * s, prod * s, mag * s.abs(), babs * s.abs()
    mrow = torch.arange(M, device=prod.device)[:, None].expand(M, N)
    ncol = torch.arange(N, device=prod.device)[None, :].expand(M, N)
    x = act_ref(x, act, nvalid, eps, mrow, ncol)
    if res is not None:
        x = x + res.double().to(prod.device)
    return x, prod, mag, babs


def check_bound(got, Ae, Be, K, *, op_term, alpha=1.0, bias=None, bias_mode=None, res=None, act=ACT_NONE, nvalid=0, eps=0.0,
                c16=False, out=None, tiny=1e-30, bias_in_acc=False, nonfinite=False, scale=None, what=None):
    """got [.., M, N] (gathered from C) against the float64 product of the effective operands Ae [.., M, K], Be [.., N, K].
    op_term: the operand-precision / accumulation coefficient of |A| |B|^T.  nonfinite=True: got must be NaN exactly where the
    reference is, +-inf with the reference's sign where it is infinite, and finite and inside the bound elsewhere.
    Returns the worst err / tol."""
    x, prod, mag, babs = reference(Ae, Be, alpha=alpha, bias=bias, bias_mode=bias_mode, res=res, act=act, nvalid=nvalid, eps=eps,
                                   scale=scale)
    tol = op_term * (mag + babs if bias_in_acc else mag) + 2.0 ** -22 * (x.abs() + prod.abs()) + tiny
    if act == ACT_ELU:
        tol = tol + 4e-6 * x.abs()
    if c16:  # rounding of the 16-bit output
        tol = tol + 2.0 ** -8 * x.abs()
    if out:
        tol = tol + out * x.abs()
    g = got.double().to(x.device)
    err = (g - x).abs()
    if not nonfinite:
        assert torch.isfinite(got).all(), what
        worst = (err / tol).max().item()
        assert worst <= 1.0, (worst, what)
        return worst
    xnan, xinf = torch.isnan(x), torch.isinf(x)
    assert xnan.any() and xinf.any(), "the non-finite case plants none"
    assert torch.equal(torch.isnan(g), xnan), (what, int(torch.isnan(g).sum()), int(xnan.sum()))
    assert torch.equal(g[xinf], x[xinf]), what
    fin = ~(xnan | xinf)
    assert torch.isfinite(g[fin]).all(), what
    # a finite result behind a non-finite product (a column RELU_EPS zeroes): no magnitude to scale a bound with, so exact
    tol = torch.where(torch.isnan(tol), torch.zeros_like(tol), tol)
    ok = fin & torch.isfinite(tol) & (tol > 0)
    worst = (err[ok] / tol[ok]).max().item() if ok.any() else 0.0
    assert (err[fin] <= tol[fin]).all() and worst <= 1.0, (worst, what)
    return worst
