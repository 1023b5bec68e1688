"""The row-op oracle (tests/rowops_oracle.py) checked on its own, without a GPU: every float64 form against naive Python
loops over the formulas of include/rfmi.h and, where it applies, against F.layer_norm / F.instance_norm / softmax in float64 on
the gathered operands; the storage builders; and the sharpness of compare(): the rounded float32 evaluation passes, four
planted faults do not."""
import math

import pytest
import torch
import torch.nn.functional as F

import rowops_oracle as O

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


def _st(off, seed, dtype=F32, scale=1.0, shift=0.0):
    return O.image_storage(off, O.randn(tuple(off.shape), seed) * scale + shift, dtype)


# ------------------------------------------------------------------------------------------------ forms against loops
@pytest.mark.parametrize("groups,act,affine", [(1, O.ACT_NONE, True), (3, O.ACT_LEAKY, True), (1, O.ACT_RELU, False)])
def test_layernorm_form(groups, act, affine):
    rows, D, x_ld, x_off, eps = 5, 7, 9, O.PAD + 3, 1e-5
    xs = _st(O.row_offsets(x_off, x_ld, rows, D), 1, shift=2.0)
    g = O.randn((groups * D,), 2).float() if affine else None
    b = O.randn((groups * D,), 3).float() if affine else None
    got = O.layernorm(xs, x_off, x_ld, rows, D, g, b, eps, groups, act, dtype=F64)
    e = O.f32(eps)
    for r in range(rows):
        v = [xs[x_off + r * x_ld + c].item() for c in range(D)]
        mean = sum(v) / D
        var = sum((t - mean) ** 2 for t in v) / D
        for c in range(D):
            y = (v[c] - mean) / math.sqrt(var + e)
            if affine:
                y = y * g[(r % groups) * D + c].item() + b[(r % groups) * D + c].item()
            if act == O.ACT_RELU:
                y = max(y, 0.0)
            if act == O.ACT_LEAKY:
                y = y if y > 0 else 0.01 * y
            assert abs(got[r, c].item() - y) < 1e-12
    if groups == 1 and act == O.ACT_NONE:
        x = xs[O.row_offsets(x_off, x_ld, rows, D)].double()
        assert torch.allclose(got, F.layer_norm(x, (D,), g.double(), b.double(), e), atol=1e-12, rtol=0)


def test_sym_layernorm_form():
    B, L, D, off = 2, 3, 5, O.PAD
    ps = _st(O.row_offsets(off, D, B * L * L, D), 4)
    got = O.sym_layernorm(ps, off, B, L, D, 1e-5, dtype=F64).reshape(B, L, L, D)
    p = ps[off:off + B * L * L * D].double().reshape(B, L, L, D)
    ref = F.layer_norm(0.5 * (p + p.transpose(1, 2)), (D,), None, None, O.f32(1e-5))
    assert torch.allclose(got, ref, atol=1e-12, rtol=0)
    for b in range(B):
        for i in range(L):
            for j in range(L):
                v = [0.5 * (ps[off + ((b * L + i) * L + j) * D + c].item() + ps[off + ((b * L + j) * L + i) * D + c].item()) for c in range(D)]
                mean = sum(v) / D
                var = sum((t - mean) ** 2 for t in v) / D
                assert abs(got[b, i, j, 2].item() - (v[2] - mean) / math.sqrt(var + O.f32(1e-5))) < 1e-12


@pytest.mark.parametrize("act,res,centre", [(O.ACT_NONE, False, False), (O.ACT_ELU, True, False), (O.ACT_NONE, False, True)])
def test_instnorm_form(act, res, centre):
    B, HW, C, off, eps = 2, 6, 3, O.PAD + 1, 1e-6
    xs = _st(O.row_offsets(off, C, B * HW, C), 5, shift=1.5)
    g, bt = (None, None) if centre else (O.randn((C,), 6).float(), O.randn((C,), 7).float())
    r = O.randn((B, HW, C), 8).float() if res else None
    got = O.instnorm(xs, off, B, HW, C, g, bt, eps, r, act, dtype=F64)
    sums, absum = O.instnorm_stats(xs, off, B, HW, C)
    for b in range(B):
        for c in range(C):
            v = [xs[off + (b * HW + p) * C + c].item() for p in range(HW)]
            mean = sum(v) / HW
            var = sum((t - mean) ** 2 for t in v) / HW
            assert abs(sums[b, c, 0].item() - sum(v)) < 1e-12 and abs(sums[b, c, 1].item() - sum(t * t for t in v)) < 1e-12
            assert abs(absum[b, c, 0].item() - sum(abs(t) for t in v)) < 1e-12
            for p in range(HW):
                y = v[p] - mean if centre else (v[p] - mean) / math.sqrt(var + O.f32(eps)) * g[c].item() + bt[c].item()
                if res:
                    y += r[b, p, c].item()
                if act == O.ACT_ELU and y <= 0:
                    y = math.expm1(y)
                assert abs(got[b, p, c].item() - y) < 1e-12
    if not centre and not res and act == O.ACT_NONE:
        x = xs[off:off + B * HW * C].double().reshape(B, HW, C).permute(0, 2, 1)
        ref = F.instance_norm(x, weight=g.double(), bias=bt.double(), eps=O.f32(eps)).permute(0, 2, 1)
        assert torch.allclose(got, ref, atol=1e-12, rtol=0)
    k = O.instnorm_kappa(xs, off, B, HW, C)
    x = xs[off:off + B * HW * C].double().reshape(B, HW, C)
    assert abs(k - (1 + x.mean(1) ** 2 / x.var(1, unbiased=False)).max().item()) < 1e-9


def test_softmax_form():
    nb, rows, cols, x_bs, x_rs, x_cs, off, scale = 2, 3, 5, 100, 1, 4, O.PAD + 2, 0.17
    xs = _st(O.strided_offsets(off, (x_bs, x_rs, x_cs), (nb, rows, cols)), 9, scale=4.0)
    got = O.softmax(xs, off, x_bs, x_rs, x_cs, rows, cols, scale, nb, dtype=F64)
    s = O.f32(scale)
    for z in range(nb):
        for r in range(rows):
            v = [s * xs[off + z * x_bs + r * x_rs + c * x_cs].item() for c in range(cols)]
            e = [math.exp(t - max(v)) for t in v]
            for c in range(cols):
                assert abs(got[z, r, c].item() - e[c] / sum(e)) < 1e-14
    x = xs[O.strided_offsets(off, (x_bs, x_rs, x_cs), (nb, rows, cols))].double()
    assert torch.allclose(got, torch.softmax(s * x, -1), atol=1e-14, rtol=0)
    a = O.softmax_allowance(O.softmax_logits(xs, off, x_bs, x_rs, x_cs, rows, cols, scale, nb, dtype=F64))
    assert (a > 0).all() and (a < 40 * 2.0 ** -23 * got + 1e-30).all()


def test_tied_sym_form():
    att = O.randn((2, 3, 4, 4), 10)
    got = O.tied_sym(att)
    for b, h, i, j in [(0, 0, 1, 2), (1, 2, 3, 0), (1, 1, 2, 2)]:
        assert got[b, i, j, h].item() == 0.5 * (att[b, h, i, j].item() + att[b, h, j, i].item())


def test_poswise_form():
    B, N, L, H, dlen, q0_ld, k_ld, k_col0, k_hs, scale = 2, 3, 2, 2, 4, 11, 13, 3, 5, 0.5
    q_off, k_off = O.PAD, O.PAD + 1
    q0s = _st(O.strided_offsets(q_off, (L * q0_ld, q0_ld, dlen, 1), (B, L, H, dlen)), 11)
    ks = _st(O.strided_offsets(k_off + k_col0, (N * L * k_ld, L * k_ld, k_ld, k_hs, 1), (B, N, L, H, dlen)), 12)
    args = (q0s, q_off, q0_ld, ks, k_off, k_ld, k_col0, k_hs, dlen, B, N, L, H, scale)
    w = O.poswise(*args, dtype=F64)
    assert w.shape == (B, N, H, L)
    for b in range(B):
        for l in range(L):
            for h in range(H):
                lg = []
                for n in range(N):
                    kb = ((b * N + n) * L + l) * k_ld + k_col0 + h * k_hs
                    qb = (b * L + l) * q0_ld + h * dlen
                    lg.append(scale * sum(q0s[q_off + qb + c].item() * ks[k_off + kb + c].item() for c in range(dlen)))
                e = [math.exp(t - max(lg)) for t in lg]
                for n in range(N):
                    assert abs(w[b, n, h, l].item() - e[n] / sum(e)) < 1e-13
    qs = O.randn((B, N, L, H, 3), 13)
    out = O.poswise_qscale(qs, w, 0.25, dtype=F64)
    assert abs(out[1, 2, 1, 0, 2].item() - qs[1, 2, 1, 0, 2].item() * w[1, 2, 0, 1].item() * 0.25) < 1e-15


def test_weighted_sum_favor_linattn_forms():
    B, N, L, D = 2, 3, 2, 5
    xs = _st(O.row_offsets(O.PAD, D, B * N * L, D), 14)
    ws = _st(O.row_offsets(O.PAD, L, B * N, L), 15)
    got = O.weighted_msa_sum(xs, O.PAD, ws, O.PAD, B, N, L, D, dtype=F64)
    for b, l, c in [(0, 0, 0), (1, 1, 4), (1, 0, 2)]:
        ref = sum(ws[O.PAD + (b * N + n) * L + l].item() * xs[O.PAD + ((b * N + n) * L + l) * D + c].item() for n in range(N))
        assert abs(got[b, l, c].item() - ref) < 1e-13
    # FAVOR+ features: both layouts, both forms
    S, n, m, m_pad, dh, n1, n2, eps = 4, 3, 5, 8, 4, 2, 2, 1e-4
    xstr = (1000, 300, 50, 7)
    for transposed in (0, 1):
        for is_query in (0, 1):
            doff = O.favor_offsets(O.PAD, S, n, m_pad, transposed)
            ds = _st(doff, 16)
            s = O.ar(S, "cpu")
            xb = (s // (n2 * n1)) * xstr[0] + ((s // n2) % n1) * xstr[1] + (s % n2) * xstr[2]
            xo = O.PAD + xb[:, None, None] + O.ar(n, "cpu")[None, :, None] * xstr[3] + O.ar(dh, "cpu")
            xs2 = _st(xo, 17)
            got = O.favor_features(ds, O.PAD, xs2, O.PAD, xstr, n1, n2, S, n, m, m_pad, dh, is_query, transposed, eps=eps, dtype=F64)
            assert got.shape == (S, n, m_pad) and (got[..., m:] == 0).all()
            for Si, r, f in [(0, 0, 0), (3, 2, 4), (2, 1, 3)]:
                s2, s1, s0 = Si % n2, (Si // n2) % n1, Si // (n2 * n1)
                base = O.PAD + Si * n * m_pad
                dv = lambda rr, ff: ds[base + (ff * n + rr if transposed else rr * m_pad + ff)].item()  # noqa: E731
                xr = [xs2[O.PAD + s0 * xstr[0] + s1 * xstr[1] + s2 * xstr[2] + r * xstr[3] + c].item() for c in range(dh)]
                diag = 0.5 * sum(t * t for t in xr) * dh ** -0.5
                mx = max(dv(r, ff) for ff in range(m)) if is_query else max(dv(rr, ff) for rr in range(n) for ff in range(m))
                ref = m ** -0.5 * (math.exp(dv(r, f) - diag - mx) + O.f32(eps))
                assert abs(got[Si, r, f].item() - ref) < 1e-13
    ns = _st(O.row_offsets(O.PAD, 9, 4, 6), 18, shift=3.0)
    got = O.linattn_normalize(ns, O.PAD, 9, 4, 5, dtype=F64)
    assert abs(got[3, 2].item() - ns[O.PAD + 3 * 9 + 2].item() / ns[O.PAD + 3 * 9 + 5].item()) < 1e-15


def test_elementwise_forms():
    x, z, w = O.randn((12,), 19).float(), O.randn((12,), 20).bfloat16(), O.randn((3,), 21).float()
    assert torch.equal(O.axpby(x, 0.5, z, -2.0, dtype=F64), 0.5 * x.double() - 2.0 * z.double())
    assert torch.equal(O.axpby(x, 0.5, None, 0.0, dtype=F64), 0.5 * x.double())
    assert torch.equal(O.scale_rows(x.reshape(3, 4), w, dtype=F64)[2, 1], x[9].double() * w[2].double())
    t = O.tile_1d_feats(O.randn((2 * 3 * 2,), 22).float(), 2, 3, 2)
    m1 = O.randn((2 * 3 * 2,), 22).float().reshape(2, 3, 2)
    assert t.shape == (2, 3, 3, 4) and t[1, 2, 0, 1] == m1[1, 2, 1] and t[1, 2, 0, 3] == m1[1, 0, 1]
    off = O.strided_offsets(5, (100, 1, 10, 0), (2, 3, 4, 1))
    assert off.shape == (2, 3, 4, 1) and off[1, 2, 3, 0].item() == 5 + 100 + 2 + 30
    assert [O.generic_code(d) for d in (1, 64, 65, 128, 129, 320, 321, 384, 385, 512, 513, 1024, 1025, 2304)] == \
        [10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 16, 16]
    assert O.generic_code(96, sym=True) == 21


# ------------------------------------------------------------------------------------------------ storage
def test_storage_builders():
    rows, D, ld, off = 4, 5, 8, O.PAD + 2
    o = O.row_offsets(off, ld, rows, D)
    st = O.image_storage(o, O.randn((rows, D), 1), BF16)
    inside = ~O.outside_image(st, o)
    assert st.numel() == off + (rows - 1) * ld + D + O.PAD
    assert torch.isnan(st[~inside]).all() and torch.isfinite(st[inside]).all() and int(inside.sum()) == rows * D
    assert torch.isnan(st[off + D]) and torch.isnan(st[off - 1]) and torch.isnan(st[off + rows * ld])  # gap, front, row past rows
    for dt in (F32, BF16, torch.float16):
        y0 = O.out_storage(o, dt)
        y = y0.clone()
        y[o.reshape(-1)] = 1.0
        O.assert_untouched(y0, y, o)
        y[off + D] = 1.0  # one stray write into the gap column
        with pytest.raises(AssertionError, match="outside the image"):
            O.assert_untouched(y0, y, o)
        y[off + D] = 0.0
        O.assert_untouched(y0, y, o, zero_off=torch.tensor([off + D]))
        y[off + D] = -0.0
        with pytest.raises(AssertionError, match="zero pad"):
            O.assert_untouched(y0, y, o, zero_off=torch.tensor([off + D]))
    with pytest.raises(AssertionError):
        O.out_storage(torch.tensor([O.PAD, O.PAD]), F32)


# ------------------------------------------------------------------------------------------------ compare
ROWS, D, LD = 9, 288, 292


@pytest.fixture(scope="module")
def ln_case():
    off = O.PAD
    xs = O.image_storage(O.row_offsets(off, LD, ROWS, D), O.randn((ROWS, D), 30) + 8.0 * O.randn((ROWS, 1), 31), F32)
    g, b = (1 + 0.1 * O.randn((D,), 32)).float(), (0.1 * O.randn((D,), 33)).float()
    r64, r32 = O.both(O.layernorm, F32, xs, off, LD, ROWS, D, g, b, 1e-5)
    return xs, off, g, b, r64, r32


@pytest.mark.parametrize("out_dtype", [F32, BF16, torch.float16])
def test_compare_accepts_the_float32_evaluation(ln_case, out_dtype):
    xs, off, g, b, _, _ = ln_case
    r64, r32 = O.both(O.layernorm, out_dtype, xs, off, LD, ROWS, D, g, b, 1e-5)
    rec = O.compare("self", r32, r64, r32)
    assert all(abs(rec[k]["ratio"] - 1 / O.FACTOR) < 1e-12 for k in ("l2", "row", "elem"))
    # F.layer_norm in float32 is another summation order of the same formula: inside the bound too
    x = xs[O.row_offsets(off, LD, ROWS, D)]
    O.compare("aten", F.layer_norm(x, (D,), g, b, O.f32(1e-5)).to(out_dtype), r64, r32)


def _rejected(name, got, r64, r32, metrics):
    rec = O.compare(name, got, r64, r32, check=False)
    for k in metrics:
        assert rec[k]["ratio"] > 1.0, (name, k, rec[k])
    with pytest.raises(AssertionError):
        O.compare(name, got, r64, r32)
    return rec


def test_compare_rejects_swapped_gamma_and_beta(ln_case):
    xs, off, g, b, r64, r32 = ln_case
    g2, b2 = g.clone(), b.clone()
    g2[17], b2[17] = b[17], g[17]  # one column of 288
    _rejected("swap", O.layernorm(xs, off, LD, ROWS, D, g2, b2, 1e-5, dtype=F32), r64, r32, ("elem", "row", "l2"))


def test_compare_rejects_one_element_off_by_one_percent(ln_case):
    _, _, _, _, r64, r32 = ln_case
    got = r32.clone()
    i = r64[4].abs().argmax()
    got[4, i] *= 1.01
    rec = _rejected("1pct", got, r64, r32, ("elem", "row"))
    # the whole-tensor relative maximum of tests/test_kernels_gpu.py lets it through at its 16-bit tolerance
    assert ((got - r64).abs().max() / r64.abs().max()).item() < 1e-2 and rec["elem"]["ratio"] > 100


def test_compare_rejects_a_row_with_its_neighbours_mean(ln_case):
    xs, off, g, b, r64, r32 = ln_case
    x = xs[O.row_offsets(off, LD, ROWS, D)]
    got = r32.clone()
    d = x[8] - x[7].mean()  # the tail row centred with the mean of the row before it
    got[8] = d / torch.sqrt((d * d).mean() + O.f32(1e-5)) * g + b
    _rejected("mean", got, r64, r32, ("row", "elem"))


def test_compare_rejects_transposed_strides():
    rows, cols, off = 5, 9, O.PAD
    x_rs, x_cs = 1, 12  # a transposed read of a [cols, 12] buffer
    xs = O.image_storage(O.strided_offsets(off, (x_rs, x_cs), (rows, cols)), 4.0 * O.randn((rows, cols), 34), F32)
    r64, r32 = O.both(O.softmax, F32, xs, off, 0, x_rs, x_cs, rows, cols, 1.0)
    xs_dense = torch.nan_to_num(xs, nan=0.0)  # the faulty kernel may read the gaps: give it numbers there
    got = O.softmax(xs_dense, off, 0, x_cs, x_rs, rows, cols, 1.0, dtype=F32)
    _rejected("transposed", got, r64, r32, ("elem", "row", "l2"))
    # and on the NaN storage the same fault is a stray read
    with pytest.raises(AssertionError, match="stray read"):
        O.compare("transposed-nan", O.softmax(xs, off, 0, x_cs, x_rs, rows, cols, 1.0, dtype=F32), r64, r32)


def test_compare_exact_and_degenerate():
    x = O.randn((3, 8), 35).float()
    r64 = x.double()
    O.compare("copy", x.bfloat16(), r64, O.rnd(r64, BF16), exact=True)
    with pytest.raises(AssertionError, match="rounded once"):
        bad = x.bfloat16()
        bad[1, 1] = bad[1, 1] * 1.01
        O.compare("copy-bad", bad, r64, O.rnd(r64, BF16), exact=True)
    with pytest.raises(AssertionError, match="declare the comparison exact"):
        O.compare("copy-undeclared", x, r64, r64)
    with pytest.raises(AssertionError, match="reference is not finite"):
        O.compare("nan-ref", x, r64 * float("nan"), r64)
