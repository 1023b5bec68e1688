"""The fused FAVOR+ kernels (csrc/favor.hip) and the tied-attention kernels (csrc/tied.hip) against the float64 oracle of
tests/attn_oracle.py: per element, per route, in both 16-bit builds.  Operands are NaN outside the image of the documented
addressing (gaps, rows past the length, PAD elements before and after), outputs a sentinel, the instantiation is asserted through
rf_attn_last_route, and each of l2 / row / elem is held to FACTOR x the error of the staged evaluation plus the derived
allowances (attn_oracle's docstring).  Every comparison prints one `[attn]` line (pytest -s); with RF_ATTN_RECORD=<path> the worst
line of every (entry point, route, build) is written there as JSON (profiles/r11_attention_bound.json).
The existing attention tests keep the guard, neighbour, run-to-run and capture checks; only the value comparison is new here."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import attn_oracle as A  # noqa: E402
import rosettafold_pytorch_amd as R  # noqa: E402,F401
from rosettafold_pytorch_amd import ops, _lib as L_  # noqa: E402
from grad_oracle import h16  # noqa: E402,F401  (the fixture: both 16-bit builds)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lib = L_.lib
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
P = ops.ptr
EINVAL, EALIGN = -1, -2
FOUR = os.environ.get("RF_FAVOR4") is not None  # read once per process by the library: this process runs the 4-wave kernels
CHILD = os.environ.get("RF_ATTN_FAVOR4_CHILD") is not None
NCU = torch.cuda.get_device_properties(0).multi_processor_count
T0 = time.time()


def dn(dt):
    return {torch.bfloat16: "bf16", torch.float16: "fp16"}[dt]


def ok(rc):
    assert rc == 0, rc


def i4(v):
    return C.byref(L_.I64x4(*[int(x) for x in v]))


def i3(v):
    return C.byref(L_.I64x3(*[int(x) for x in v]))


@pytest.fixture(scope="module", autouse=True)
def record():
    yield
    path = os.environ.get("RF_ATTN_RECORD")
    if not path:
        return

    def sig(v):
        return v if v is None or isinstance(v, (str, bool)) else float("%.4g" % v)
    groups = {}
    for c in A.ATTN_RECORDS:
        groups.setdefault((c["case"].split("/")[0], str(c["route"]), c["build"]), []).append(c)
    lines = []
    for (op, route, build), cs in sorted(groups.items()):
        g = dict(op=op, route=route, build=build, n=len(cs))
        for m in ("l2", "row", "elem"):
            w = max(cs, key=lambda c: c[m]["ratio"])
            g[m] = [sig(w[m][k]) for k in ("err", "e32", "extra", "ratio")]
        g["worst_elem_case"] = max(cs, key=lambda c: c["elem"]["ratio"])["case"]
        lines.append(json.dumps(g))
    child = path + ".favor4"  # the groups of the 4-wave child process (test_four_wave_kernels_in_a_fresh_process)
    if not CHILD and os.path.exists(child):
        with open(child) as fh:
            lines += [json.dumps(g) for g in json.load(fh)["groups"]]
        os.remove(child)
    info = {"planted_faults_rejected_by_the_bf16_staging": A.planted_faults(torch.bfloat16),
            "planted_faults_rejected_by_the_fp16_staging": A.planted_faults(torch.float16),
            "module_wall_seconds": round(time.time() - T0, 1)}
    with open(path, "w") as fh:
        fh.write('{"factor": %g, "comparisons": %d, "columns": ["err", "staged", "extra", "err / bound"],\n"info": %s,\n"groups": [\n%s\n]}\n' % (
            A.FACTOR, len(A.ATTN_RECORDS), json.dumps(info), ",\n".join(lines)))


# ================================================================================================ rf_favor_attention
SM_LENGTHS = [1, 17, 63, 64, 65, 100, 128, 129, 200, 255, 256]
RELU_LENGTHS = SM_LENGTHS + [257, 300, 512, 513, 700]
_PC = {}


def proj(sm, h):
    if (sm, h) not in _PC:
        _PC[sm, h] = A.projection(17, sm, h, DEV)
    return _PC[sm, h]


def run_favor(name, layout, n_b, n_o, n_h, S, sm, h, *, std=1.0, vm=0.0, seed=0):
    c = A.favor_case(layout, n_b, n_o, n_h, S, qk_std=std, v_mean=vm, seed=seed, h16=h, device=DEV)
    pc, eps = proj(sm, h), (1e-4 if sm else 1e-3)
    a = (c["qkv"], pc) + c["args"] + (sm, eps)
    r64, off, d64 = A.favor_attention(*a, dtype=F64, detail=True)
    st, _ = A.favor_attention(*a, dtype=F32, h16=h)
    oo = off + A.PAD
    o0 = A.out_storage(oo, h)
    os_ = o0.clone()
    ok(lib.rf_favor_attention(P(c["qkv"], A.PAD), P(pc), P(os_, A.PAD), i4(c["xs"]), i3(c["os"]), *c["cols"], n_b, n_o, n_h, S, 64, 266,
                              int(sm), eps, ops.stream()))
    code = A.favor_code(S, sm, FOUR)
    assert lib.rf_attn_last_route() == code, (name, lib.rf_attn_last_route(), code)
    torch.cuda.synchronize()
    A.assert_untouched(o0, os_, oo, what=name)
    # (one key: out is v itself.  The 16-bit roundings of the context move the ratio by 2^-9 / sqrt(266) at most, far inside half
    # a unit of the stored value, so every correct evaluation stores exactly v: the comparison is declared exact)
    return A.check(f"favor/{name}/{layout}/{n_b}x{n_o}x{n_h}/S{S}/std{std}/vm{vm}", os_[oo], r64, st, A.favor_extra(r64, d64),
                   route=code, build=dn(h), exact=S == 1)


@pytest.mark.parametrize("sm,S", [(True, n) for n in SM_LENGTHS] + [(False, n) for n in RELU_LENGTHS])
def test_favor_attention_small_item_counts(h16, sm, S):
    """1 and 3 items at every length, both layouts of test_favor_ragged_gpu._layout, q / k of unit variance and of standard
    deviation 2 (softmax map: a wide exponent range, many features at eps), v zero-mean and with mean 4 sigma"""
    nm = "softmax" if sm else "relu"
    run_favor(nm, "contiguous", 1, 1, 1, S, sm, h16, std=1.0, vm=0.0, seed=S)
    run_favor(nm, "contiguous", 1, 1, 3, S, sm, h16, std=2.0, vm=4.0, seed=S + 1)
    run_favor(nm, "strided", 1, 3, 1, S, sm, h16, std=1.0, vm=4.0, seed=S + 2)
    run_favor(nm, "strided", 1, 3, 1, S, sm, h16, std=2.0, vm=0.0, seed=S + 3)
    if S in (17, 100, 256, 300):
        run_favor(nm, "headmajor", 1, 1, 3, S, sm, h16, std=1.0, vm=0.0, seed=S + 4)


@pytest.mark.parametrize("sm,S", [(sm, n) for sm in (True, False) for n in (64, 60, 128, 100, 256, 200)] + [(False, 512), (False, 300)])
def test_favor_attention_full_machine(h16, sm, S):
    """multi_processor_count + 14 items (rounded up to whole triples of heads): every workgroup is resident, 14 of them walk a
    second item with the next item's K / V prefetch in flight behind phase B, one aligned and one tail length per tile size"""
    n_o = (NCU + 14 + 2) // 3
    run_favor("full-" + ("softmax" if sm else "relu"), "contiguous", 1, n_o, 3, S, sm, h16, std=2.0 if S in (60, 128, 200) else 1.0,
              vm=4.0 if S in (64, 100, 512) else 0.0, seed=S)


def test_four_wave_kernels_in_a_fresh_process():
    """RF_FAVOR4 is read once per process: the favor cases and the route table once more in a child pytest of this module with
    the switch set; there every route code must say 4-wave (run_favor asserts it against favor_code(.., four_wave=True))"""
    assert not CHILD, "the child selects its tests with -k and never starts a child of its own"
    env = dict(os.environ, RF_FAVOR4="1", RF_ATTN_FAVOR4_CHILD="1")
    if env.get("RF_ATTN_RECORD"):
        env["RF_ATTN_RECORD"] += ".favor4"
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s",
                        "-p", "no:cacheprovider", "-k", "favor_attention or route_code"], env=env, cwd=ROOT, capture_output=True, text=True)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    print(tail)
    assert r.returncode == 0, (r.returncode, tail)
    routes = {ln.split("route=")[1].split()[0] for ln in r.stdout.splitlines() if ln.startswith("[attn] favor/")}
    assert routes and all(x.startswith("favor4_") for x in routes), routes
    assert routes == {v for k, v in A.ROUTES.items() if 100 <= k < 112}, routes


# ================================================================================================ tied logits
TIED_LENGTHS = [1, 17, 63, 64, 65, 100, 128, 129, 191, 192, 193, 255, 256]
TILES = (64, 128, 192, 256)


def padded_ld(L):
    return (L + 1 + 7) // 8 * 8


def run_logits(name, B, H, N, L, h, *, att_ld=None, with_w=False, spread=4.0, workspace=False, entry="ld", seed=0):
    att_ld = att_ld or L
    c = A.tied_case(B, H, N, L, with_w=with_w, spread=spread, seed=seed, h16=h, device=DEV, rowmajor=entry == "softmax")
    a = (c["q"], c["k"], c["st"], c["w"], c["ws"], c["qscale"], B, H, N, L, att_ld)
    r64, d64 = A.tied_logits(*a, dtype=F64, detail=True)
    st = A.tied_logits(*a, dtype=F32, h16=h)
    sym_ld = H + 3
    ao, zo, so = A.att_offsets(A.PAD, B, H, L, att_ld, DEV), A.att_pad_offsets(A.PAD, B, H, L, att_ld, DEV), A.sym_offsets(A.PAD, B, H, L, sym_ld, DEV)
    a0 = A.out_storage(torch.cat([ao.reshape(-1), zo.reshape(-1)]) if zo is not None else ao, h)
    s0 = A.out_storage(so, F32)
    as_, ss = a0.clone(), s0.clone()
    ws_elems = ((4 if N > 128 else 2) if L == 256 else 1) * B * H * L * L if workspace else 0
    ws = torch.full((ws_elems,), float("nan"), device=DEV) if workspace else None
    q, k, att, sym, w = P(c["q"], A.PAD), P(c["k"], A.PAD), P(as_, A.PAD), P(ss, A.PAD), P(c["w"], A.PAD) if with_w else None
    wst = i3(c["ws"]) if with_w else None
    if entry == "softmax":  # rf_tied_logits_softmax: rows holding all heads, q already scaled
        ok(lib.rf_tied_logits_softmax(q, k, c["st"][0], c["st"][1], c["st"][3], att, sym, sym_ld, B, H, N, L, 32, ops.stream()))
    elif entry == "plain":
        ok(lib.rf_tied_logits(q, k, i4(c["st"]), w, wst, c["qscale"], att, sym, sym_ld, B, H, N, L, 32, P(ws), ws_elems, ops.stream()))
    else:
        ok(lib.rf_tied_logits_ld(q, k, i4(c["st"]), w, wst, c["qscale"], att, att_ld, sym, sym_ld, B, H, N, L, 32, P(ws), ws_elems,
                                 ops.stream()))
    split = workspace and att_ld == L and A.split_applies(L, N, ws_elems, B, H)
    code = A.split_code(L, with_w) if split else A.logits_code(L, att_ld, with_w)
    assert lib.rf_attn_last_route() == code, (name, lib.rf_attn_last_route(), code)
    torch.cuda.synchronize()
    A.assert_untouched(a0, as_, ao, zero_off=zo, what=name)  # (the pad columns [L, att_ld) hold exact zeros)
    A.assert_untouched(s0, ss, so, what=name)
    att_v, sym_v = as_[ao], ss[so]
    rec = A.check(f"tied_logits/{name}/{entry}/B{B}H{H}N{N}L{L}/ld{att_ld}/w{int(with_w)}/spread{spread}/ws{int(workspace)}", att_v, r64, st,
                  A.tied_logits_extra(d64, N), route=code, build=dn(h), exact=L == 1)
    s64 = A.tied_sym(att_v)  # 0.5 * (a + b) of two stored 16-bit values is one fp32 rounding: exact
    assert torch.equal(sym_v.to(F64), A.rnd(s64, F32)), (name, "att_sym is not the symmetrisation of the stored att")
    assert torch.equal(sym_v, sym_v.transpose(1, 2)), (name, "att_sym is not bitwise symmetric")
    return rec, code


@pytest.mark.parametrize("N", [1, 5, 16, 37, 130])
@pytest.mark.parametrize("L", TIED_LENGTHS)
def test_tied_logits(h16, L, N):
    """every length with att_ld = L where that is legal and att_ld = 8 ceil((L + 1) / 8), H = 1 and 3, logit spreads of about 4
    and about 30, w == NULL and (where the library takes it: N % 4 == 0) w given with NaN in the row pad"""
    for i, (H, ld, spread) in enumerate([(1, L if L % 8 == 0 else padded_ld(L), 4.0), (3, padded_ld(L), 30.0), (3, L if L % 8 == 0 else padded_ld(L), 30.0)]):
        run_logits("onepass", 2, H, N, L, h16, att_ld=ld, spread=spread, seed=L + N + i)
        if N % 4 == 0:
            run_logits("onepass", 2, H, N, L, h16, att_ld=ld, with_w=True, spread=34.0 - spread, seed=L + N + i)
    if L in TILES:
        run_logits("onepass", 2, 3, N, L, h16, spread=4.0, entry="plain", with_w=N % 4 == 0, seed=L)
        run_logits("onepass", 2, 3, N, L, h16, spread=30.0, entry="softmax", seed=L)


@pytest.mark.parametrize("N,H", [(8, 3), (128, 3), (256, 1)])
def test_tied_logits_contraction_split(h16, N, H):
    """L = 256 with a workspace: N = 8 (4 MSA rows per range), 128 (two ranges of 64), 256 (four ranges)"""
    for with_w in (False, True):
        _, code = run_logits("split", 2, H, N, 256, h16, with_w=with_w, spread=4.0 if with_w else 30.0, workspace=True, seed=N)
        assert code == 220 + int(with_w)
    _, code = run_logits("split", 2, H, N, 256, h16, spread=4.0, workspace=True, entry="plain", seed=N + 1)
    assert code == 220


@pytest.mark.parametrize("N", [130, 5])
def test_tied_logits_split_falls_back_to_the_one_pass_kernel(h16, N):
    """130 = 2 x 65 rows per range and an odd N are outside the split kernel: with the workspace given the one-pass kernel runs"""
    _, code = run_logits("fallback", 2, 1, N, 256, h16, spread=4.0, workspace=True, seed=N)
    assert code == 212
    _, code = run_logits("fallback", 2, 1, N, 256, h16, att_ld=264, spread=30.0, workspace=True, seed=N)  # (not dense: never split)
    assert code == 213


@pytest.mark.parametrize("N", [4, 16])
@pytest.mark.parametrize("L", [512, 768, 1024])
def test_tied_logits_long_rows(h16, L, N):
    _, code = run_logits("long", 1, 1, N, L, h16, spread=4.0 if N == 4 else 30.0, workspace=True, seed=L + N)
    assert code == 220 + 2 * (L // 256 - 1)


# ================================================================================================ attention . V
def stored_att(B, H, L, att_ld, spread, seed, h):
    """a float64 softmax rounded to the build type, the pad columns exact zeros; (storage, offsets, pad offsets)"""
    ao, zo = A.att_offsets(A.PAD, B, H, L, att_ld, DEV), A.att_pad_offsets(A.PAD, B, H, L, att_ld, DEV)
    att = torch.softmax(spread / 5.0 * A.randn((B, H, L, L), seed, DEV), -1)
    if zo is None:
        return A.image_storage(ao, att, h), ao, zo
    return A.image_storage(torch.cat([ao.reshape(-1), zo.reshape(-1)]), torch.cat([att.reshape(-1), torch.zeros(zo.numel(), dtype=F64, device=DEV)]), h), ao, zo


def run_av(name, B, H, N, L, h, *, att_ld=None, rowmajor=False, spread=4.0, entry="ld", seed=0):
    att_ld = att_ld or L
    c = A.tied_case(B, H, N, L, with_w=False, spread=1.0, seed=seed, h16=h, device=DEV, rowmajor=rowmajor)
    ast, _, _ = stored_att(B, H, L, att_ld, spread, seed + 7, h)
    a = (ast, att_ld, c["v"], c["st"], c["st"], B, H, N, L)
    r64, off = A.tied_av(*a, dtype=F64)
    st, _ = A.tied_av(*a, dtype=F32, h16=h)
    oo = off + A.PAD
    o0 = A.out_storage(oo, h)
    os_ = o0.clone()
    if entry == "plain":
        ok(lib.rf_tied_av(P(ast, A.PAD), P(c["v"], A.PAD), i4(c["st"]), P(os_, A.PAD), i4(c["st"]), B, H, N, L, 32, ops.stream()))
    else:
        ok(lib.rf_tied_av_ld(P(ast, A.PAD), att_ld, P(c["v"], A.PAD), i4(c["st"]), P(os_, A.PAD), i4(c["st"]), B, H, N, L, 32, ops.stream()))
    code = A.av_code(L, att_ld)
    assert lib.rf_attn_last_route() == code, (name, lib.rf_attn_last_route(), code)
    torch.cuda.synchronize()
    A.assert_untouched(o0, os_, oo, what=name)
    return A.check(f"tied_av/{name}/{entry}/B{B}H{H}N{N}L{L}/ld{att_ld}/rm{int(rowmajor)}/spread{spread}", os_[oo], r64, st, route=code,
                   build=dn(h), exact=L == 1)


@pytest.mark.parametrize("L", TIED_LENGTHS)
def test_tied_av(h16, L):
    dense = L if L % 8 == 0 else padded_ld(L)
    run_av("av", 2, 3, 5, L, h16, att_ld=dense, rowmajor=False, spread=4.0, seed=L)
    run_av("av", 2, 3, 5, L, h16, att_ld=padded_ld(L), rowmajor=True, spread=30.0, seed=L + 1)
    run_av("av", 1, 1, 1, L, h16, att_ld=padded_ld(L), rowmajor=False, spread=30.0, seed=L + 2)
    if L in TILES:
        run_av("av", 2, 1, 3, L, h16, rowmajor=True, spread=4.0, entry="plain", seed=L + 3)


@pytest.mark.parametrize("L", [64, 100])
@pytest.mark.parametrize("units", [1, 7, 0])
def test_tied_av_unit_counts(h16, L, units):
    """B * H * N = 1, 7 and 2 * multi_processor_count + 1: with the last the workgroups walk two units and the last one walks one"""
    N = units or 2 * NCU + 1
    run_av(f"units{N}", 1, 1, N, L, h16, att_ld=L if L % 8 == 0 else padded_ld(L), spread=4.0, seed=N)


# ================================================================================================ the composition
@pytest.mark.parametrize("workspace", [False, True], ids=["nows", "ws"])
@pytest.mark.parametrize("L", [100, 256])
def test_tied_attention(h16, L, workspace):
    """rf_tied_attention(_ld): att against the logits form, out against attention . V of the STORED att and against the
    end-to-end float64 value"""
    h, B, H, N = h16, 2, 3, 8
    for with_w, att_ld, entry in [(True, padded_ld(L) if L % 8 else L, "ld"), (False, padded_ld(L), "ld")] + ([(True, L, "plain")] if L == 256 else []):
        c = A.tied_case(B, H, N, L, with_w=with_w, spread=4.0 if with_w else 30.0, seed=L + int(with_w), h16=h, device=DEV)
        a = (c["q"], c["k"], c["st"], c["w"], c["ws"], c["qscale"], B, H, N, L, att_ld)
        a64, d64 = A.tied_logits(*a, dtype=F64, detail=True)
        ast = A.tied_logits(*a, dtype=F32, h16=h)
        ao, zo = A.att_offsets(A.PAD, B, H, L, att_ld, DEV), A.att_pad_offsets(A.PAD, B, H, L, att_ld, DEV)
        a0 = A.out_storage(torch.cat([ao.reshape(-1), zo.reshape(-1)]) if zo is not None else ao, h)
        oo = A.qk_offsets(A.PAD, c["st"], B, N, H, L, DEV)
        o0 = A.out_storage(oo, h)
        as_, os_ = a0.clone(), o0.clone()
        ws_elems = 2 * B * H * L * L if workspace else 0
        ws = torch.full((ws_elems,), float("nan"), device=DEV) if workspace else None
        args = (P(c["q"], A.PAD), P(c["k"], A.PAD), P(c["v"], A.PAD), i4(c["st"]), i4(c["st"]), P(c["w"], A.PAD) if with_w else None,
                i3(c["ws"]) if with_w else None, c["qscale"], P(as_, A.PAD))
        rest = (None, 0, P(os_, A.PAD), i4(c["st"]), B, H, N, L, 32, P(ws), ws_elems, ops.stream())
        ok(lib.rf_tied_attention(*args, *rest) if entry == "plain" else lib.rf_tied_attention_ld(*args, att_ld, *rest))
        split = workspace and att_ld == L and A.split_applies(L, N, ws_elems, B, H)
        lcode, vcode = A.split_code(L, with_w) if split else A.logits_code(L, att_ld, with_w), A.av_code(L, att_ld)
        assert lib.rf_attn_last_route() == 1000 * lcode + vcode, (lib.rf_attn_last_route(), lcode, vcode)
        torch.cuda.synchronize()
        A.assert_untouched(a0, as_, ao, zero_off=zo)
        A.assert_untouched(o0, os_, oo)
        nm = f"L{L}/ld{att_ld}/w{int(with_w)}/ws{int(workspace)}/{entry}"
        lextra = A.tied_logits_extra(d64, N)
        A.check(f"tied_attention/att/{nm}", as_[ao], a64, ast, lextra, route=lcode, build=dn(h))
        # out against attention . V of the stored att
        va = (as_, att_ld, c["v"], c["st"], c["st"], B, H, N, L)
        o64, _ = A.tied_av(*va, dtype=F64)
        ost, _ = A.tied_av(*va, dtype=F32, h16=h)
        A.check(f"tied_attention/out_of_stored_att/{nm}", os_[oo], o64, ost, route=vcode, build=dn(h))
        # end to end: float64 att . v; staged: the staged att through the staged attention . V; the att allowances through |v|
        vv = c["v"][oo].to(F64)
        e64 = torch.einsum("bhij,bnhjd->bnhid", a64, vv)
        est = A.rnd(torch.einsum("bhij,bnhjd->bnhid", ast.to(F32), vv.to(F32)), h)
        A.check(f"tied_attention/out_end_to_end/{nm}", os_[oo], e64, est, torch.einsum("bhij,bnhjd->bnhid", lextra, vv.abs()),
                route=1000 * lcode + vcode, build=dn(h))


# ================================================================================================ rf_poswise_collapsed
def run_poswise(B, N, L, D, H, spread, h, seed=0):
    scale = spread / 5.0 / D ** 0.5
    xo = A.strided_offsets(A.PAD, (N * L * D, L * D, D, 1), (B, N, L, D), DEV)
    uo = A.strided_offsets(A.PAD, (L * H * D, H * D, D, 1), (B, L, H, D), DEV)
    xn = A.image_storage(xo, A.randn((B, N, L, D), seed, DEV), h)
    u = A.image_storage(uo, A.randn((B, L, H, D), seed + 1, DEV), h)
    a = (xn, u, B, N, L, D, H, scale)
    r64, d64 = A.poswise_collapsed(*a, dtype=F64, detail=True)
    st = A.poswise_collapsed(*a, dtype=F32, h16=h)
    wo = A.poswise_offsets(A.PAD, B, H, N, L, DEV)
    w0 = A.out_storage(wo, F32)
    ws = w0.clone()
    ok(lib.rf_poswise_collapsed(P(xn, A.PAD), P(u, A.PAD), P(ws, A.PAD), B, N, L, D, H, scale, ops.stream()))
    code = A.poswise_code(N)
    assert lib.rf_attn_last_route() == code, (lib.rf_attn_last_route(), code)
    torch.cuda.synchronize()
    A.assert_untouched(w0, ws, wo)
    got, extra = ws[wo], A.poswise_extra(d64, D)
    rec = A.check(f"poswise_collapsed/B{B}N{N}L{L}D{D}H{H}/spread{spread}", got, r64, st, extra, route=code, build=dn(h))
    # rows sum to 1 within the softmax allowance and the roundings of the fp32 row sum (N - 1 additions), of 1 / sum and of the
    # products with it
    assert ((got.to(F64).sum(-1) - 1).abs() <= extra.sum(-1) + (N + 4) * 2.0 ** -24).all()
    return rec


@pytest.mark.parametrize("H", [1, 12, 16])
@pytest.mark.parametrize("N", [16, 48, 256])
def test_poswise_collapsed(h16, N, H):
    i = 0
    for D in (32, 96, 384):
        for L in (1, 5, 20):
            run_poswise(2, N, L, D, H, 30.0 if i % 2 else 4.0, h16, seed=N + H + i)
            i += 1


# ================================================================================================ argument checks
def test_rejected_arguments(h16):
    """values only: every call returns before a launch"""
    h = h16
    z = torch.zeros(1 << 16, device=DEV, dtype=h)
    zf = torch.zeros(1 << 16, device=DEV)
    s = ops.stream()

    def favor(S, sm, xs=(0, 0, 192, 64)):
        return lib.rf_favor_attention(P(z), P(z), P(z), i4(xs), i3((0, 0, 64)), 0, 64, 128, 1, 1, 1, S, 64, 266, sm, 1e-3, s)
    assert favor(257, 1) == EINVAL
    assert favor(64, 0, (0, 0, 196, 64)) == EALIGN and favor(64, 0, (0, 0, 192, 68)) == EALIGN
    st = (8 * 64 * 32, 64 * 32, 64 * 32, 32)

    def logits(L, att_ld):
        return lib.rf_tied_logits_ld(P(z), P(z), i4(st), None, None, 1.0, P(z), att_ld, None, 0, 1, 1, 8, L, 32, None, 0, s)

    def av(L, att_ld):
        return lib.rf_tied_av_ld(P(z), att_ld, P(z), i4(st), P(z), i4(st), 1, 1, 8, L, 32, s)

    def attention(L, att_ld):
        return lib.rf_tied_attention_ld(P(z), P(z), P(z), i4(st), i4(st), None, None, 1.0, P(z), att_ld, None, 0, P(z), i4(st), 1, 1, 8, L,
                                        32, None, 0, s)
    for f in (logits, av, attention):
        assert f(40, 32) == EINVAL and f(40, 44) == EALIGN, f.__name__
    assert lib.rf_tied_logits_ld(P(z), P(z), i4((8 * 64 * 32, 64 * 32 + 4, 64 * 32, 32)), None, None, 1.0, P(z), 64, None, 0, 1, 1, 8, 64, 32,
                                 None, 0, s) == EALIGN
    assert lib.rf_poswise_collapsed(P(z), P(z), P(zf), 1, 272, 4, 32, 4, 1.0, s) == EINVAL
    assert lib.rf_poswise_collapsed(P(z), P(z), P(zf), 1, 16, 4, 32, 17, 1.0, s) == EINVAL
    torch.cuda.synchronize()
    assert not z.any() and not zf.any()


# ================================================================================================ the route table
def test_every_route_code_is_reached(h16):
    """One small case per code of rf_attn_last_route that this process can reach (each asserts its code and goes through the same
    comparison): the 8-wave FAVOR+ codes and the two 4-wave ones of the 256-row softmax tile here, all twelve 4-wave codes in the
    RF_FAVOR4 child (test_four_wave_kernels_in_a_fresh_process); together they are the table of include/rfmi.h, which
    tests/test_attn_oracle_cpu.py holds equal to attn_oracle.ROUTES."""
    h = h16
    witness = {}
    for sm in (False, True):
        for S in (64, 60, 128, 100, 256, 200):
            witness[A.favor_code(S, sm, FOUR)] = lambda sm=sm, S=S: run_favor("w", "contiguous", 1, 1, 3, S, sm, h, seed=S)
    for i, T in enumerate(TILES):
        for with_w in (False, True):
            witness[200 + 4 * i + 2 * int(with_w)] = lambda T=T, w=with_w: run_logits("w", 1, 1, 4, T, h, with_w=w, seed=T)
            witness[201 + 4 * i + 2 * int(with_w)] = lambda T=T, w=with_w: run_logits("w", 1, 1, 4, T - 3, h, att_ld=T, with_w=w, seed=T)
        witness[240 + 2 * i] = lambda T=T: run_av("w", 1, 1, 2, T, h, seed=T)
        witness[241 + 2 * i] = lambda T=T: run_av("w", 1, 1, 2, T, h, att_ld=T + 8, seed=T)
    witness[220] = lambda: run_logits("w", 1, 1, 8, 256, h, workspace=True)
    witness[221] = lambda: run_logits("w", 1, 1, 8, 256, h, with_w=True, workspace=True)
    for L in (512, 768, 1024):
        witness[220 + 2 * (L // 256 - 1)] = lambda L=L: run_logits("w", 1, 1, 4, L, h, workspace=True)
    for nt in (1, 2, 3, 4, 5, 6, 7, 8, 12, 16):
        witness[260 + nt] = lambda nt=nt: run_poswise(1, 16 * nt, 3, 32, 2, 4.0, h, seed=nt)
    other = {A.favor_code(S, sm, not FOUR) for sm in (False, True) for S in (64, 60, 128, 100, 256, 200)}
    assert set(witness) | other == set(A.ROUTES), sorted((set(witness) | other) ^ set(A.ROUTES))
    assert FOUR == all(k < 112 for k in witness if k < 200)
    for code in sorted(witness):
        witness[code]()
        assert lib.rf_attn_last_route() == code
