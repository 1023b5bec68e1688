"""The GEMM oracle (tests/gemm_oracle.py) checked on its own, without a GPU: its index-tensor offset formulas against naive
Python loops over the formulas of include/rfmi.h, and the sharpness of the per-element bound -- a stand-in "kernel" (the CPU
fp32 product of bf16-rounded operands) passes it, and each planted indexing error exceeds it by at least 10x."""
import pytest
import torch

import gemm_oracle as O


# ------------------------------------------------------------------------------------------------ the header, as loops
def _split(i, rc, ro, ri):
    return (i // rc) * ro + (i % rc) * ri if rc > 0 else i * ri


def naive(d, Ast, Bst):
    """A[z][m][k], B[z][n][k] and the C offsets by the header's formulas, one element at a time"""
    Z = d["nb0"] * d["nb1"] * d["nb2"]
    M, N, K, kc = d["M"], d["N"], d["K"], d["kc"]
    A, B = torch.zeros(Z, M, K, dtype=torch.float64), torch.zeros(Z, N, K, dtype=torch.float64)
    Coff = torch.zeros(Z, M, N, dtype=torch.int64)
    for z0 in range(d["nb0"]):
        for z1 in range(d["nb1"]):
            for z2 in range(d["nb2"]):
                z = (z0 * d["nb1"] + z1) * d["nb2"] + z2
                za, zb, zc = (z0 * d[s][0] + z1 * d[s][1] + z2 * d[s][2] for s in ("a_bs", "b_bs", "c_bs"))
                for m in range(M):
                    for k in range(K):
                        if d["a_mode"] == O.AMODE_CONV3X3:
                            h, w, c, dil = d["conv_h"], d["conv_w"], d["conv_c"], d["conv_dil"]
                            tap, ch = k // c, k % c
                            img, pix = m // (h * w), m % (h * w)
                            i, j = pix // w + (tap // 3 - 1) * dil, pix % w + (tap % 3 - 1) * dil
                            if 0 <= i < h and 0 <= j < w:
                                A[z, m, k] = Ast[d["a_off"] + ((img * h + i) * w + j) * c + ch]
                        else:
                            A[z, m, k] = Ast[d["a_off"] + za + _split(m, d["a_rc"], d["a_ro"], d["a_ri"]) + (k // kc) * d["a_ko"] + k % kc]
                    for n in range(N):
                        Coff[z, m, n] = zc + _split(m, d["c_rc"], d["c_ro"], d["c_ri"]) + _split(n, d["c_cc"], d["c_co"], 1)
                for n in range(N):
                    for k in range(K):
                        B[z, n, k] = Bst[d["b_off"] + zb + _split(n, d["b_rc"], d["b_ro"], d["b_ri"]) + (k // kc) * d["b_ko"] + k % kc]
    return A, B, Coff


def _cases():
    M, N, K = 7, 5, 16
    yield "plain", O.desc(M, N, K)
    yield "padded_rows", O.desc(M, N, K, a_ri=K + 8, b_ri=K + 16, c_ri=N + 3)
    # three-level batch (2, 3, 1), B broadcast over the middle level (b_bs[1] = 0)
    yield "batch_broadcast", O.desc(M, N, K, nb0=2, nb1=3, nb2=1, a_bs=(3 * M * K, M * K, 0), b_bs=(N * K, 0, 0),
                                    c_bs=(3 * M * N, M * N, 0))
    yield "batch_inner", O.desc(M, N, K, nb0=2, nb1=1, nb2=2, a_bs=(2 * M * K, 0, M * K), b_bs=(0, 0, N * K),
                                c_bs=(2 * M * N + 8, 0, M * N))
    # rows in groups of 3 with 2 padding rows, both operands
    yield "split_rows", O.desc(9, 6, K, a_rc=3, a_ro=5 * K, b_rc=3, b_ro=5 * (K + 8), b_ri=K + 8)
    # K in chunks of 8 with 8-element gaps; kc that does not divide K evenly into the row (kc = 8 of K = 24 with gap 16)
    yield "k_chunks", O.desc(M, N, 24, kc=8, a_ko=16, a_ri=48, b_ko=24, b_ri=72)
    yield "split_c_pow2", O.desc(8, 16, K, c_rc=4, c_ro=6 * 8, c_ri=8, c_cc=8, c_co=2 * 6 * 8)
    yield "split_c_odd", O.desc(9, 12, K, c_rc=3, c_ro=5 * 4, c_ri=4, c_cc=4, c_co=3 * 5 * 4 + 8)
    for dil in (1, 2, 4):  # dilation >= h and >= w included
        yield f"conv_dil{dil}", O.desc(2 * 3 * 4, 5, 9 * 8, a_mode=O.AMODE_CONV3X3, conv_n=2, conv_h=3, conv_w=4, conv_c=8,
                                      conv_dil=dil, b_ri=9 * 8)
    yield "pointer_offsets", O.desc(M, N, K, a_off=O.PAD + 8, b_off=O.PAD + 8, c_off=O.PAD + 1)


CASES = dict(_cases())


@pytest.mark.parametrize("name", list(CASES))
def test_offsets_equal_the_headers_formulas(name):
    d = CASES[name]
    Ast, Bst = O.make_operand(d, "a", torch.float32, 1), O.make_operand(d, "b", torch.float32, 2)
    A, B = O.effective_operands(d, Ast, Bst)
    An, Bn, Cn = naive(d, Ast, Bst)
    assert torch.equal(A, An) and torch.equal(B, Bn)
    assert torch.isfinite(A).all() and torch.isfinite(B).all()
    assert torch.equal(O.c_offsets(d), Cn)
    # every element the formulas do not reach is NaN, PAD of them at either end
    for st, side in ((Ast, "a"), (Bst, "b")):
        off, valid = O.operand_offsets(d, side)
        reached = torch.zeros(st.numel(), dtype=torch.bool)
        reached[off[valid] + d[side + "_off"]] = True
        assert torch.isnan(st[~reached]).all() and torch.isfinite(st[reached]).all()
        assert not reached[:O.PAD].any() and not reached[-O.PAD:].any()
    if name == "conv_dil4":  # dilation beyond the picture: only the centre tap is inside
        assert (A[:, :, :4 * 8] == 0).all() and (A[:, :, 5 * 8:] == 0).all()


def test_c_storage_sentinels():
    d = CASES["split_c_odd"]
    C0 = O.make_c(d, torch.float32)
    C = C0.clone()
    img = O.c_offsets(d) + d["c_off"]
    C[img.reshape(-1)] = 1.0
    O.assert_untouched(d, C0, C)
    assert torch.equal(O.gather_c(d, C), torch.ones(1, d["M"], d["N"]))
    assert img.numel() < C.numel() - 2 * O.PAD  # the layout has gaps, and they hold the sentinel
    image = set(img.reshape(-1).tolist())
    gap_row = d["c_off"] + 3 * 4  # rows 3 and 4 of every group of 5 are padding
    for stray in (0, O.PAD - 1, int(img.max()) + 1, C.numel() - 1, gap_row):
        assert stray not in image
        Cb = C.clone()
        Cb[stray] = 0.0
        with pytest.raises(AssertionError):
            O.assert_untouched(d, C0, Cb)
    Cb = C.clone()
    Cb[gap_row] = torch.tensor(-1234.0).nextafter(torch.tensor(0.0))  # one bit away from the sentinel
    with pytest.raises(AssertionError):
        O.assert_untouched(d, C0, Cb)


# ------------------------------------------------------------------------------------------------ sharpness of the bound
def _fake(K, seed=0):
    """a stand-in kernel: bf16-rounded operands, fp32 product on the CPU, fp32 bias"""
    M, N = 40, 24
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g).bfloat16()
    B = torch.randn(N, K, generator=g).bfloat16()
    bias = torch.randn(N, generator=g)
    C = A.float() @ B.float().t() + bias
    return A, B, bias, C


def _worst(C, A, B, bias, K):
    return O.check_bound(C, A, B, K, op_term=O.op_term_h16(K), bias=bias, bias_in_acc=True)


def _plant(kind, A, B, bias, C):
    C = C.clone()
    K = A.shape[1]
    if kind == "dropped_k_chunk":  # one 8-element K chunk missing from one column
        n, k0 = 5, 8 * (K // 16)
        C[:, n] -= A[:, k0:k0 + 8].float() @ B[n, k0:k0 + 8].float()
    elif kind == "swapped_columns":
        C[:, [3, 4]] = C[:, [4, 3]]
    elif kind == "row_from_row_above":
        m = 17
        C[m] = A[m - 1].float() @ B.float().t() + bias
    elif kind == "bias_twice":
        C += bias
    elif kind == "stored_one_row_low":
        C[12, 7] = C[11, 7]
    else:
        raise KeyError(kind)
    return C


@pytest.mark.parametrize("K", [288, 1152])
def test_bound_passes_the_clean_product(K):
    A, B, bias, C = _fake(K)
    w = _worst(C, A, B, bias, K)
    print(f"\n[gemm oracle] K={K}: clean fp32 product of bf16 operands, worst err / tol = {w:.3f}")
    assert w <= 1.0
    with pytest.raises(AssertionError):  # a 16-bit output needs its rounding term, and passes with it
        _worst(C.bfloat16().float(), A, B, bias, K)
    O.check_bound(C.bfloat16(), A, B, K, op_term=O.op_term_h16(K), bias=bias, bias_in_acc=True, out=O.OUT_ROUND[torch.bfloat16])


@pytest.mark.parametrize("kind", ["dropped_k_chunk", "swapped_columns", "row_from_row_above", "bias_twice", "stored_one_row_low"])
@pytest.mark.parametrize("K", [288, 1152])
def test_bound_is_sharp(K, kind):
    A, B, bias, C = _fake(K)
    bad = _plant(kind, A, B, bias, C)
    with pytest.raises(AssertionError) as e:
        _worst(bad, A, B, bias, K)
    worst = e.value.args[0][0]
    print(f"\n[gemm oracle] K={K} {kind}: worst err / tol = {worst:.1f}")
    assert worst >= 10.0, (kind, K, worst)


def test_nonfinite_mode():
    K = 32
    A, B, bias, _ = _fake(K)
    A, B = A.float(), B.float()
    A[3, 5], A[10, 1], B[7, 2] = float("inf"), float("-inf"), float("nan")
    C = A @ B.t() + bias
    O.check_bound(C, A, B, K, op_term=O.op_term_h16(K), bias=bias, bias_in_acc=True, nonfinite=True)
    O.check_bound(torch.relu(C), A, B, K, op_term=O.op_term_h16(K), bias=bias, bias_in_acc=True, act=O.ACT_RELU, nonfinite=True)
    swallowed = torch.where(torch.isnan(C), torch.full_like(C, float("-inf")), C)  # what fmaxf(acc, -inf) makes of a NaN
    with pytest.raises(AssertionError):
        O.check_bound(swallowed, A, B, K, op_term=O.op_term_h16(K), bias=bias, bias_in_acc=True, nonfinite=True)
    zeroed = torch.relu(C).nan_to_num(nan=0.0, posinf=float("inf"))  # what fmaxf(v, 0) makes of it
    with pytest.raises(AssertionError):
        O.check_bound(zeroed, A, B, K, op_term=O.op_term_h16(K), bias=bias, bias_in_acc=True, act=O.ACT_RELU, nonfinite=True)
