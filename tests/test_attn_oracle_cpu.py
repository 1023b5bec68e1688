"""tests/attn_oracle.py checked without a GPU: every form against naive Python loops at tiny shapes, the route helpers against
the table of include/rfmi.h, the staged evaluation against itself summed in another order (the bound must not reject a correct
kernel) and six planted value faults (it must reject a wrong one)."""
import math
import os
import re

import pytest
import torch

import attn_oracle as A

F64, F32 = torch.float64, torch.float32
H16 = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]


# ------------------------------------------------------------------------------------------------ forms against loops
@pytest.mark.parametrize("softmax_kernel", [False, True], ids=["relu", "softmax"])
@pytest.mark.parametrize("layout", ["contiguous", "strided", "headmajor"])
def test_favor_attention_against_loops(layout, softmax_kernel):
    n_b, n_o, n_h, S, eps = 1, 2, 2, 3, 1e-3
    c = A.favor_case(layout, n_b, n_o, n_h, S, seed=3, h16=torch.bfloat16)
    pc = A.projection(2, softmax_kernel, torch.bfloat16)
    out, off = A.favor_attention(c["qkv"], pc, *c["args"], softmax_kernel, eps, dtype=F64)
    st, P, e = c["qkv"].double().tolist(), pc.double().tolist(), A.f32(eps)
    xs, os_, (qc, kc, vc) = c["xs"], c["os"], c["cols"]
    for b in range(n_b):
        for o in range(n_o):
            for h in range(n_h):
                def row(col, s):
                    base = A.PAD + col + b * xs[0] + o * xs[1] + s * xs[2] + h * xs[3]
                    return st[base:base + 64]

                def logits(x):
                    return [sum(x[d] * P[m][d] for d in range(64)) for m in range(A.FV_M)]

                def diag(x):
                    return sum(t * t for t in x) * 64 ** -0.5 * A.LOG2E / 2
                lk = [logits(row(kc, s)) for s in range(S)]
                kmax = max(max(r) for r in lk)
                for s in range(S):
                    lq = logits(row(qc, s))
                    if softmax_kernel:
                        qp = [2.0 ** (t - diag(row(qc, s)) - max(lq)) + e for t in lq]
                        kp = [[2.0 ** (t - diag(row(kc, j)) - kmax) + e for t in lk[j]] for j in range(S)]
                    else:
                        qp = [max(t, 0.0) + e for t in lq]
                        kp = [[max(t, 0.0) + e for t in lk[j]] for j in range(S)]
                    wts = [sum(qp[m] * kp[j][m] for m in range(A.FV_M)) for j in range(S)]
                    for d in range(0, 64, 7):
                        want = sum(wts[j] * row(vc, j)[d] for j in range(S)) / sum(wts)
                        assert abs(out[b, o, h, s, d].item() - want) <= 1e-12 * max(1.0, abs(want)), (b, o, h, s, d)
                        assert off[b, o, h, s, d].item() == b * os_[0] + o * os_[1] + s * os_[2] + h * 64 + d


@pytest.mark.parametrize("with_w", [False, True], ids=["noscale", "scale"])
def test_tied_forms_against_loops(with_w):
    B, H, N, L, att_ld = 2, 2, 2, 5, 8
    c = A.tied_case(B, H, N, L, with_w=with_w, spread=4.0, seed=1, h16=torch.float16)
    att = A.tied_logits(c["q"], c["k"], c["st"], c["w"], c["ws"], c["qscale"], B, H, N, L, att_ld, dtype=F64)
    q, k, v = (c[n].double().tolist() for n in "qkv")
    w = c["w"].double().tolist() if with_w else None
    s, qs = c["st"], A.f32(c["qscale"])

    def el(t, b, n, h, l, d):
        return t[A.PAD + b * s[0] + n * s[1] + h * s[2] + l * s[3] + d]
    for b in range(B):
        for h in range(H):
            for i in range(L):
                lg = []
                for j in range(L):
                    a = 0.0
                    for n in range(N):
                        f = w[A.PAD + b * c["ws"][0] + h * c["ws"][1] + n * c["ws"][2] + i] * qs if with_w else 1.0
                        a += sum(f * el(q, b, n, h, i, d) * el(k, b, n, h, j, d) for d in range(32))
                    lg.append(a)
                z = sum(math.exp(t - max(lg)) for t in lg)
                for j in range(L):
                    assert abs(att[b, h, i, j].item() - math.exp(lg[j] - max(lg)) / z) < 1e-13
    # attention . V from a stored att with row pitch att_ld, and the placement helpers
    ao = A.att_offsets(A.PAD, B, H, L, att_ld)
    zo = A.att_pad_offsets(A.PAD, B, H, L, att_ld)
    assert ao[1, 1, 4, 4].item() == A.PAD + ((1 * H + 1) * L + 4) * att_ld + 4
    assert zo.shape == (B * H * L, att_ld - L) and not set(zo.reshape(-1).tolist()) & set(ao.reshape(-1).tolist())
    assert A.att_pad_offsets(A.PAD, B, H, L, L) is None
    ast = A.image_storage(ao, att, torch.float16)
    out, off = A.tied_av(ast, att_ld, c["v"], c["st"], c["st"], B, H, N, L, dtype=F64)
    al = ast.double().tolist()
    for b in range(B):
        for n in range(N):
            for h in range(H):
                for i in range(L):
                    for d in (0, 13, 31):
                        want = sum(al[ao[b, h, i, j].item()] * el(v, b, n, h, j, d) for j in range(L))
                        assert abs(out[b, n, h, i, d].item() - want) < 1e-13
                        assert off[b, n, h, i, d].item() == b * s[0] + n * s[1] + h * s[2] + i * s[3] + d
    sym = A.tied_sym(ast[ao])
    assert sym.shape == (B, L, L, H) and sym[1, 2, 3, 1].item() == 0.5 * (al[ao[1, 1, 2, 3].item()] + al[ao[1, 1, 3, 2].item()])


def test_poswise_collapsed_against_loops():
    B, N, L, D, H, scale = 2, 2, 5, 32, 3, 0.31
    xo = A.strided_offsets(A.PAD, (N * L * D, L * D, D, 1), (B, N, L, D))
    uo = A.strided_offsets(A.PAD, (L * H * D, H * D, D, 1), (B, L, H, D))
    xn = A.image_storage(xo, A.randn((B, N, L, D), 1), torch.bfloat16)
    u = A.image_storage(uo, A.randn((B, L, H, D), 2), torch.bfloat16)
    w = A.poswise_collapsed(xn, u, B, N, L, D, H, scale, dtype=F64)
    x, uu, sc = xn.double().tolist(), u.double().tolist(), A.f32(scale)
    wo = A.poswise_offsets(0, B, H, N, L)
    for b in range(B):
        for h in range(H):
            for l in range(L):
                t = [sc * sum(x[A.PAD + ((b * N + n) * L + l) * D + c] * uu[A.PAD + ((b * L + l) * H + h) * D + c] for c in range(D))
                     for n in range(N)]
                z = sum(math.exp(v - max(t)) for v in t)
                for n in range(N):
                    assert abs(w[b, h, l, n].item() - math.exp(t[n] - max(t)) / z) < 1e-13
                    assert wo[b, h, l, n].item() == ((b * H + h) * N + n) * L + l


# ------------------------------------------------------------------------------------------------ allowances, routes
def test_exp2_allowance_is_the_tighter_form():
    t = -torch.logspace(-3, 2, 200, dtype=F64)
    assert (A.exp2_allowance(t) <= A.exp_allowance(t * math.log(2.0)) * (1 + 1e-12)).all()
    assert (A.exp2_allowance(t) >= 2.0 ** -22 * torch.exp2(t)).all()
    y = torch.softmax(torch.tensor([[0.3, -1.0, 2.0]], dtype=F64), -1)
    delta = torch.tensor([[1e-3, 2e-3, 5e-4]], dtype=F64)
    moved = torch.softmax(torch.tensor([[0.3 + 1e-3, -1.0 - 2e-3, 2.0 - 5e-4]], dtype=F64), -1)
    assert ((moved - y).abs() <= A.softmax_carry(y, delta) * 1.01).all()


def test_route_table_of_the_header_lists_the_oracle_codes():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rfmi.h")).read()
    table = hdr[hdr.index("Introspection for tests and measurement tools, like rf_rowops_last_route"):hdr.index("int rf_attn_last_route")]
    listed = set()
    for line in re.findall(r"^ \*   (\d[\d ./]*?)  ", table, flags=re.M):
        if ".." in line:
            a, b = (int(x) for x in line.split(".."))
            listed |= set(range(a, b + 1))
        else:
            listed |= {int(x) for x in line.split("/")}
    assert listed == set(A.ROUTES), sorted(listed ^ set(A.ROUTES))
    assert A.favor_code(64, False) == 112 and A.favor_code(300, False) == 121 and A.favor_code(200, True) == 111
    assert A.favor_code(100, True, four_wave=True) == 107 and A.favor_code(512, False) == 120
    assert A.logits_code(100, 104, True) == 207 and A.logits_code(256, 256, False) == 212 and A.av_code(64, 72) == 241
    assert A.split_applies(256, 8, 2 * 2 * 3 * 65536, 2, 3) and not A.split_applies(256, 130, 1 << 30, 2, 3)
    assert not A.split_applies(256, 5, 1 << 30, 2, 3) and A.split_applies(1024, 4, 1 << 20, 1, 1)


# ------------------------------------------------------------------------------------------------ reordered staging
FAVOR_FAMILIES = [  # (softmax features, seq_len, q / k standard deviation, mean of v): the families of the GPU module
    (False, 17, 1.0, 0.0), (False, 100, 2.0, 4.0), (False, 300, 1.0, 4.0), (False, 700, 2.0, 0.0),
    (True, 1, 1.0, 0.0), (True, 17, 2.0, 4.0), (True, 100, 1.0, 0.0), (True, 200, 2.0, 0.0), (True, 256, 1.0, 4.0)]


@pytest.mark.parametrize("h16", H16, ids=IDS)
@pytest.mark.parametrize("sm,S,std,vm", FAVOR_FAMILIES)
def test_favor_staging_in_reversed_chunks_stays_inside_the_bound(sm, S, std, vm, h16):
    c = A.favor_case("contiguous", 1, 1, 3, S, qk_std=std, v_mean=vm, seed=S, h16=h16)
    pc = A.projection(4, sm, h16)
    eps = 1e-4 if sm else 1e-3
    a = (c["qkv"], pc) + c["args"] + (sm, eps)
    r64, _, d64 = A.favor_attention(*a, dtype=F64, detail=True)
    st, _ = A.favor_attention(*a, dtype=F32, h16=h16)
    rev, _ = A.favor_attention(*a, dtype=F32, h16=h16, seq_chunk=16)
    A.check(f"reordered/favor/{'softmax' if sm else 'relu'}/S{S}/std{std}/vm{vm}", rev, r64, st, A.favor_extra(r64, d64), build=str(h16))


@pytest.mark.parametrize("h16", H16, ids=IDS)
@pytest.mark.parametrize("with_w", [False, True], ids=["noscale", "scale"])
@pytest.mark.parametrize("L,N,spread", [(17, 4, 4.0), (100, 16, 30.0), (64, 128, 4.0), (65, 36, 30.0), (256, 8, 4.0)])
def test_tied_staging_in_two_halves_stays_inside_the_bound(L, N, spread, with_w, h16):
    B, H = 1, 2
    c = A.tied_case(B, H, N, L, with_w=with_w, spread=spread, seed=L + N, h16=h16)
    a = (c["q"], c["k"], c["st"], c["w"], c["ws"], c["qscale"], B, H, N, L, L)
    r64, d64 = A.tied_logits(*a, dtype=F64, detail=True)
    st = A.tied_logits(*a, dtype=F32, h16=h16)
    halves = A.tied_logits(*a, dtype=F32, h16=h16, n_halves=True)
    A.check(f"reordered/logits/L{L}/N{N}/spread{spread}/w{int(with_w)}", halves, r64, st, A.tied_logits_extra(d64, N), build=str(h16))


# ------------------------------------------------------------------------------------------------ planted faults
def test_planted_faults_are_rejected():
    res = A.planted_faults(torch.float16)
    assert sorted(res) == sorted(A.PLANTED)
    assert all(res.values()), res
    print("planted faults the bf16 staging rejects too (information):", A.planted_faults(torch.bfloat16))
