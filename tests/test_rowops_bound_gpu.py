"""Every norm, softmax and element-wise kernel of csrc/ops.hip against the float64 oracle of tests/rowops_oracle.py: per
element, per route, in both 16-bit builds.  Inputs are NaN outside the image of the op's addressing, outputs a sentinel, the
route is asserted through rf_rowops_last_route, and each of l2 / row / elem is held to FACTOR x the error of the rounded float32
evaluation (times kappa for InstanceNorm's one-pass variance, plus the fast-exponential allowance where a kernel uses __expf);
the derivations are in rowops_oracle's docstring.  Every comparison prints one `[rowops]` line (pytest -s); with
RF_ROWOPS_RECORD=<path> the worst line of every (op, route) is written there as JSON (profiles/r09_rowops_bound.json)."""
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import rowops_oracle as O  # noqa: E402
from grad_oracle import h16  # noqa: E402,F401  (the fixture: both 16-bit builds)
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import ops, _lib as L  # noqa: E402

lib = L.lib
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
P = ops.ptr
EINVAL, EALIGN = -1, -2
INFO = {}  # measurements that are recorded, not asserted (the InstanceNorm sweep, the model's mean/sigma)


@pytest.fixture(scope="module", autouse=True)
def record():
    yield
    path = os.environ.get("RF_ROWOPS_RECORD")
    if path:  # one line per (op, route): the number of comparisons and, per metric, the one with the largest err / bound
        def sig(v):
            return v if v is None or isinstance(v, (str, bool)) else float("%.4g" % v)

        def walk(v):
            return {k: walk(x) for k, x in v.items()} if isinstance(v, dict) else sig(v)

        groups = {}
        for c in O.RECORDS:
            groups.setdefault((c["case"].split("/")[0], c["route"]), []).append(c)
        lines = []
        for (op, route), cs in sorted(groups.items(), key=lambda kv: (kv[0][0], str(kv[0][1]))):
            g = dict(op=op, route=route, n=len(cs), kappa_max=sig(max(c["kappa"] for c in cs)))
            for m in ("l2", "row", "elem"):
                w = max(cs, key=lambda c: c[m]["ratio"])
                g[m] = [sig(w[m][k]) for k in ("err", "e32", "extra", "ratio")]
            g["worst_elem_case"] = max(cs, key=lambda c: c["elem"]["ratio"])["case"]
            lines.append(json.dumps(g))
        with open(path, "w") as fh:
            fh.write('{"factor": %g, "comparisons": %d, "columns": ["err", "e32", "extra", "err / bound"],\n"info": {\n%s\n},\n"groups": [\n%s\n]}\n' % (
                O.FACTOR, len(O.RECORDS), ",\n".join(json.dumps(k) + ": " + json.dumps(walk(v)) for k, v in INFO.items()), ",\n".join(lines)))


def ok(rc):
    assert rc == 0, rc


def dn(dt):
    return {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "fp16"}[dt]


def rows_with_offset(rows, D, ms, seed):
    """unit-variance rows whose mean / sigma is +-ms"""
    sign = torch.where(O.randn((rows, 1), seed + 1, DEV) > 0, 1.0, -1.0)
    return O.randn((rows, D), seed, DEV) + ms * sign


# ================================================================================================ LayerNorm
LN_VARIANTS = [  # (fp32 output?, affine, act, row mean / sigma)
    (True, True, O.ACT_NONE, 0.3), (False, True, O.ACT_NONE, 8.0), (True, False, O.ACT_RELU, 40.0),
    (False, True, O.ACT_LEAKY, 40.0), (False, False, O.ACT_NONE, 0.3), (True, True, O.ACT_LEAKY, 8.0)]


def run_ln(name, rows, D, h, *, route, x16=False, y32=True, x_ld=None, y_ld=None, out_off=0, x_mis=0, g_mis=0, affine=True,
           groups=1, act=O.ACT_NONE, ms=0.3, seed=0):
    x_dt, y_dt = (h if x16 else F32), (F32 if y32 else h)
    x_ld, y_ld = x_ld or D, y_ld or D
    x_off, y_off = O.PAD + x_mis, O.PAD + out_off
    xs = O.image_storage(O.row_offsets(x_off, x_ld, rows, D, DEV), rows_with_offset(rows, D, ms, seed), x_dt)
    g = b = gs = bs = None
    if affine:  # (g_mis: gamma / beta at a pointer that is not 16-byte aligned)
        gs = torch.cat([torch.full((4 + g_mis,), float("nan"), device=DEV), (1 + 0.2 * O.randn((groups * D,), seed + 2, DEV)).float()])
        bs = torch.cat([torch.full((4 + g_mis,), float("nan"), device=DEV), (0.3 * O.randn((groups * D,), seed + 3, DEV)).float()])
        g, b = gs[4 + g_mis:], bs[4 + g_mis:]
    yo = O.row_offsets(y_off, y_ld, rows, D, DEV)
    y0 = O.out_storage(yo, y_dt)
    ys = y0.clone()
    ok(lib.rf_layernorm(P(xs, x_off), ops.dcode(x_dt), x_ld, P(ys, y_off), ops.dcode(y_dt), y_ld, rows, D,
                        P(gs, 4 + g_mis) if affine else None, P(bs, 4 + g_mis) if affine else None, 1e-5, groups, act, ops.stream()))
    assert lib.rf_rowops_last_route() == route, (name, lib.rf_rowops_last_route(), route)
    torch.cuda.synchronize()
    O.assert_untouched(y0, ys, yo, what=name)
    r64, r32 = O.both(O.layernorm, y_dt, xs, x_off, x_ld, rows, D, g, b, 1e-5, groups, act)
    exact = D == 1  # x - mean is exactly 0: the result is beta, rounded once
    return O.compare(f"layernorm/{name}/{dn(x_dt)}->{dn(y_dt)}/aff{int(affine)}/act{act}/ms{ms}", ys[yo], r64, r32, exact=exact,
                     route=O.ROUTES[route])


def ln_variants(name, rows, D, h, *, route, acts=True, **kw):
    for y32, affine, act, ms in LN_VARIANTS:
        if not acts and act != O.ACT_NONE:
            act = O.ACT_NONE
        if D == 1 and act == O.ACT_LEAKY:
            act = O.ACT_RELU  # (0.01f * beta is not the float64 product rounded once)
        run_ln(name, rows, D, h, route=route, y32=y32, affine=affine, act=act, ms=ms, **kw)


@pytest.mark.parametrize("D,route", [(288, 1), (384, 2)])
@pytest.mark.parametrize("rows", [1, 7, 33])
def test_layernorm_rows8(h16, D, route, rows):
    ln_variants(f"rows8-{D}x{rows}", rows, D, h16, route=route)
    ln_variants(f"rows8-{D}x{rows}-xld", rows, D, h16, route=route, x_ld=D + 4)
    ln_variants(f"rows8-{D}x{rows}-slice", rows, D, h16, route=route, y_ld=D + 16, out_off=8)


@pytest.mark.parametrize("D,route", [(288, 1), (384, 2)])
def test_layernorm_rows8_grid_loop(h16, D, route):
    """65536 + 40 rows: the grid is capped at 2048 workgroups of 32 rows, every wave takes a second pass and the last is ragged"""
    run_ln(f"rows8-{D}-loop", 65536 + 40, D, h16, route=route, y32=False, act=O.ACT_RELU, ms=8.0)


@pytest.mark.parametrize("D", [128, 132, 512])
@pytest.mark.parametrize("rows", [1, 3])
def test_layernorm_vec2(h16, D, rows):
    ln_variants(f"vec2-{D}x{rows}", rows, D, h16, route=5)


@pytest.mark.parametrize("D", [128, 132, 512])
def test_layernorm_vec2_grid_loop(h16, D):
    run_ln(f"vec2-{D}-loop", 16384 + 5, D, h16, route=5, y32=False, act=O.ACT_LEAKY, ms=8.0)


@pytest.mark.parametrize("D", [516, 1024])
def test_layernorm_vec4(h16, D):
    ln_variants(f"vec4-{D}", 3, D, h16, route=6)


@pytest.mark.parametrize("D", [520, 1024])
@pytest.mark.parametrize("rows", [5, 8192 + 3])
def test_layernorm_vec_h16(h16, D, rows):
    if rows == 5:
        ln_variants(f"vech16-{D}x{rows}", rows, D, h16, route=7, acts=False, x16=True)
        run_ln(f"vech16-{D}-xld", rows, D, h16, route=7, x16=True, x_ld=D + 8, y_ld=D + 8, y32=False)
    else:
        run_ln(f"vech16-{D}-loop", rows, D, h16, route=7, x16=True, y32=False, ms=8.0)


@pytest.mark.parametrize("D,route", [(32, 8), (64, 9)])
def test_layernorm_narrow(h16, D, route):
    ln_variants(f"narrow-{D}", 5, D, h16, route=route)
    for y32 in (True, False):
        run_ln(f"narrow-{D}-groups8", 21, D, h16, route=route, groups=8, act=O.ACT_LEAKY, y32=y32)


def test_layernorm_narrow_grid_loop(h16):
    run_ln("narrow-32-loop", 131072 + 9, 32, h16, route=8, y32=False, groups=8, act=O.ACT_LEAKY, ms=8.0)


@pytest.mark.parametrize("D", [1, 63, 65, 124, 130, 321, 385, 513, 1025, 2304])
def test_layernorm_generic(h16, D):
    ln_variants(f"generic-{D}", 5, D, h16, route=O.generic_code(D))


def test_layernorm_generic_forced(h16):
    """D = 288 off the fast kernels: 16-bit input, a pointer 4 bytes off 16-byte alignment (x, y, gamma in turn), x_ld = 289,
    groups; D = 1024 16-bit input with an activation leaves the 16-bit vector kernel"""
    ln_variants("generic-288-h16in", 5, 288, h16, route=12, x16=True)
    ln_variants("generic-288-xmis", 5, 288, h16, route=12, x_mis=1)
    run_ln("generic-288-ymis", 5, 288, h16, route=12, out_off=1)
    run_ln("generic-288-gmis", 5, 288, h16, route=12, g_mis=1)
    ln_variants("generic-288-xld289", 5, 288, h16, route=12, x_ld=289)
    ln_variants("generic-288-groups3", 7, 288, h16, route=12, groups=3)
    ln_variants("generic-130-groups3", 7, 130, h16, route=12, groups=3)
    run_ln("generic-1024-h16in-relu", 5, 1024, h16, route=15, x16=True, act=O.ACT_RELU, y32=False)
    run_ln("generic-132-xld133", 3, 132, h16, route=12, x_ld=133)
    run_ln("generic-32-xmis", 5, 32, h16, route=10, x_mis=2)


SYM_CASES = [(288, 3, 0), (384, 4, 0), (96, 21, 0), (100, 21, 0)]
SYM_MORE = [(40, 20, 0), (200, 22, 0), (288, 22, 1), (352, 23, 0), (500, 24, 0), (1000, 25, 0), (1100, 26, 0)]


def run_sym(D, route, mis, L_, h, y32):
    B = 2
    y_dt = F32 if y32 else h
    off = O.PAD + mis
    po = O.row_offsets(off, D, B * L_ * L_, D, DEV)
    ps = O.image_storage(po, rows_with_offset(B * L_ * L_, D, 3.0, D + L_), F32)
    yo = O.row_offsets(O.PAD, D, B * L_ * L_, D, DEV)
    y0 = O.out_storage(yo, y_dt)
    ys = y0.clone()
    ok(lib.rf_sym_layernorm(P(ps, off), P(ys, O.PAD), ops.dcode(y_dt), B, L_, D, 1e-5, ops.stream()))
    assert lib.rf_rowops_last_route() == route, (lib.rf_rowops_last_route(), route)
    torch.cuda.synchronize()
    O.assert_untouched(y0, ys, yo)
    got = ys[yo]
    r64, r32 = O.both(O.sym_layernorm, y_dt, ps, off, B, L_, D, 1e-5)
    O.compare(f"sym_layernorm/{D}/L{L_}/mis{mis}/{dn(y_dt)}", got, r64, r32, route=O.ROUTES[route])
    g4 = got.reshape(B, L_, L_, D)
    assert torch.equal(g4, g4.transpose(1, 2)), "the output is not bitwise symmetric in (i, j)"


@pytest.mark.parametrize("L_", [1, 5, 13])
@pytest.mark.parametrize("D,route,mis", SYM_CASES)
def test_sym_layernorm(h16, D, route, mis, L_):
    for y32 in (True, False):
        run_sym(D, route, mis, L_, h16, y32)


@pytest.mark.parametrize("D,route,mis", SYM_MORE)
def test_sym_layernorm_generic_instantiations(h16, D, route, mis):
    run_sym(D, route, mis, 5, h16, False)


# ================================================================================================ InstanceNorm
def in_apply_route(x_dt, C, HW, aligned, centre):
    """include/rfmi.h, rf_rowops_last_route"""
    if centre or x_dt == F32 or C % 8 or not aligned:
        return 32
    nch = C // 8
    return 34 if -(-HW * nch // 256) < nch // math.gcd(nch, 256) else 33


def run_instnorm(name, B, HW, C, h, *, x16, y32=True, y2=None, res=False, act=O.ACT_NONE, centre=False, ms=0.5, x_mis=0,
                 via_ops=False, vals=None, seed=0, check=True, routes=None):
    """rf_instnorm_stats + rf_instnorm_apply on NaN-padded x; returns (record of the output, worst sums error / bound)"""
    x_dt, y_dt = (h if x16 else F32), (F32 if y32 else h)
    y2_dt = None if y2 is None else (F32 if y2 == "f32" else h)
    off = O.PAD + x_mis
    xo = O.strided_offsets(off, (HW * C, C, 1), (B, HW, C), DEV)
    if vals is None:
        sign = torch.where(O.randn((B, 1, C), seed + 1, DEV) > 0, 1.0, -1.0)
        vals = O.randn((B, HW, C), seed, DEV) + ms * sign
    xs = O.image_storage(xo, vals, x_dt)
    g, bt = (None, None) if centre else ((1 + 0.2 * O.randn((C,), seed + 2, DEV)).float(), (0.3 * O.randn((C,), seed + 3, DEV)).float())
    r = (0.5 * O.randn((B, HW, C), seed + 4, DEV)).float() if res else None
    eps = 0.0 if centre else 1e-6
    yo = O.strided_offsets(O.PAD, (HW * C, C, 1), (B, HW, C), DEV)
    y0, y20 = O.out_storage(yo, y_dt), (O.out_storage(yo, y2_dt) if y2_dt else None)
    ys, y2s = y0.clone(), (y20.clone() if y2_dt else None)
    vec_stats = x16 and C % 8 == 0 and x_mis % 8 == 0
    want = (31 if vec_stats else 30, in_apply_route(x_dt, C, HW, x_mis % 8 == 0, centre))
    if routes is not None:
        assert want == routes, (want, routes)
    if via_ops:
        assert x_mis == 0
        x4 = xs[off:off + B * HW * C].view(B, 1, HW, C)
        stats = []
        ops.instnorm(x4, g, bt, eps=eps, residual=r.view(B, 1, HW, C) if res else None, act=act,
                     out=ys[O.PAD:O.PAD + B * HW * C].view(B, 1, HW, C),
                     out2=y2s[O.PAD:O.PAD + B * HW * C].view(B, 1, HW, C) if y2_dt else None, stats_out=stats)
        assert lib.rf_rowops_last_route() == want[1]
        sums = stats[0]
    else:
        sums = torch.full((B * C * 2 + 2,), float("nan"), device=DEV, dtype=F64)
        nws = int(lib.rf_instnorm_ws_bytes(B, HW, C))
        ws = torch.empty(nws, device=DEV, dtype=torch.uint8)
        ok(lib.rf_instnorm_stats(P(xs, off), ops.dcode(x_dt), P(sums), B, HW, C, P(ws), nws, ops.stream()))
        assert lib.rf_rowops_last_route() == want[0], (name, lib.rf_rowops_last_route(), want)
        ok(lib.rf_instnorm_apply(P(xs, off), ops.dcode(x_dt), P(sums), P(g), P(bt), eps, P(r), act, P(ys, O.PAD), ops.dcode(y_dt),
                                 P(y2s, O.PAD) if y2_dt else None, ops.dcode(y2_dt) if y2_dt else 0, B, HW, C, ops.stream()))
        assert lib.rf_rowops_last_route() == want[1], (name, lib.rf_rowops_last_route(), want)
        torch.cuda.synchronize()
        assert torch.isnan(sums[B * C * 2:]).all(), "the statistics wrote past 2*B*C doubles"
        sums = sums[:B * C * 2]
    torch.cuda.synchronize()
    # the fp64 sums: float64 additions of fp32 block partials (rowops_oracle: sums_bound)
    s64, sabs = O.instnorm_stats(xs, off, B, HW, C)
    bound = O.sums_bound(sabs, 512 if vec_stats else 128)
    serr = (sums.reshape(B, C, 2) - s64).abs()
    assert torch.isfinite(sums).all() and (serr <= bound).all(), (name, (serr / bound.clamp_min(1e-300)).max().item())
    worst_sums = (serr / bound.clamp_min(1e-300)).max().item()
    O.assert_untouched(y0, ys, yo, what=name)
    kappa = 1.0 if centre else O.instnorm_kappa(xs, off, B, HW, C)
    extra = None
    if act == O.ACT_ELU:
        extra = O.elu_allowance(O.instnorm(xs, off, B, HW, C, g, bt, eps, r, O.ACT_NONE, dtype=F64))
    tag = f"instnorm/{name}/{dn(x_dt)}->{dn(y_dt)}/res{int(res)}/act{act}/centre{int(centre)}"
    r64, r32 = O.both(O.instnorm, y_dt, xs, off, B, HW, C, g, bt, eps, r, act)
    rec = O.compare(tag, ys[yo], r64, r32, extra, kappa=kappa, route=O.ROUTES[want[0]] + "+" + O.ROUTES[want[1]], check=check)
    if y2_dt:
        O.assert_untouched(y20, y2s, yo, what=name)
        r64b, r32b = O.both(O.instnorm, y2_dt, xs, off, B, HW, C, g, bt, eps, r, act)
        O.compare(tag + "/y2-" + dn(y2_dt), y2s[yo], r64b, r32b, extra, kappa=kappa, route=O.ROUTES[want[1]], check=check)
    return rec, worst_sums, kappa


@pytest.mark.parametrize("x16", [False, True], ids=["x32", "x16"])
@pytest.mark.parametrize("HW", [9, 529, 1369, 4489])
@pytest.mark.parametrize("C", [8, 20, 72, 288])
def test_instnorm(h16, C, HW, x16):
    """less than one block of pixels, a ragged last block, and more than 8 partial blocks (4489 pixels: 36 generic / 9 vector
    blocks, so every lane group of the finalize kernel adds more than once)"""
    nm = f"C{C}-HW{HW}"
    run_instnorm(nm, 2, HW, C, h16, x16=x16, y32=False)
    run_instnorm(nm, 2, HW, C, h16, x16=x16, y32=True, y2="h16", res=True, act=O.ACT_ELU)
    run_instnorm(nm, 2, HW, C, h16, x16=x16, y32=False, y2="f32", res=True, act=O.ACT_ELU, via_ops=True)
    run_instnorm(nm, 2, HW, C, h16, x16=x16, y32=True, act=O.ACT_ELU)
    run_instnorm(nm, 2, HW, C, h16, x16=x16, y32=True, centre=True)
    run_instnorm(nm, 2, HW, C, h16, x16=x16, y32=False, centre=True, via_ops=True)


def test_instnorm_apply_index_modes(h16):
    """the vectorised apply kernel with every thread on one channel chunk (C = 72, 37 x 37) and re-deriving the chunk from the
    index (C = 72, 3 x 3: the grid stride 256 is no multiple of 9); and off the vector kernels by a pointer 4 bytes off"""
    for res, act in ((False, O.ACT_NONE), (True, O.ACT_ELU)):
        run_instnorm("fixed", 2, 1369, 72, h16, x16=True, y32=False, y2="f32", res=res, act=act, routes=(31, 33))
        run_instnorm("modulo", 2, 9, 72, h16, x16=True, y32=False, y2="f32", res=res, act=act, routes=(31, 34))
        run_instnorm("modulo-288", 2, 9, 288, h16, x16=True, y32=True, y2="h16", res=res, act=act, routes=(31, 34))
    run_instnorm("misaligned", 2, 529, 72, h16, x16=True, y32=False, x_mis=2, routes=(30, 32))


def standardised(B, HW, C, ms, seed):
    """every (b, c) with mean exactly +-ms and variance 1 (in float64, before the rounding to the input dtype)"""
    z = O.randn((B, HW, C), seed, DEV)
    z = (z - z.mean(1, keepdim=True)) / z.std(1, unbiased=False, keepdim=True)
    return z + ms * torch.where(O.randn((B, 1, C), seed + 1, DEV) > 0, 1.0, -1.0)


@pytest.mark.parametrize("x16", [False, True], ids=["x32", "x16"])
def test_instnorm_mean_over_sigma_sweep(h16, x16):
    """Per-channel mean / sigma in {0, 1, 4, 8, 32}: the one-pass variance loses 1 + mean^2 / var, the bound carries exactly
    that (kappa, capped at 2 for the first two); the ratio to the float32 evaluation without kappa is recorded."""
    B, HW, C = 2, 1369, 72
    sweep = {}
    for ms in (0, 1, 4, 8, 32):
        rec, worst_sums, kappa = run_instnorm(f"sweep-ms{ms}", B, HW, C, h16, x16=x16, y32=True, vals=standardised(B, HW, C, ms, 50 + ms),
                                              check=False)
        if ms <= 1:
            assert kappa <= 2 * (1 + 2.0 ** -6), kappa  # (2 before the rounding of x to its dtype)
            kappa = min(kappa, 2.0)
        for k in ("l2", "row", "elem"):
            assert rec[k]["err"] <= O.FACTOR * kappa * rec[k]["e32"], (ms, k, rec[k], kappa)
        sweep[str(ms)] = dict(kappa=kappa, sums=worst_sums, **{k: rec[k]["ratio_e32"] for k in ("l2", "row", "elem")})
    INFO[f"instnorm_sweep/{dn(h16)}/{'x16' if x16 else 'x32'}"] = sweep


def test_instnorm_mean_over_sigma_in_the_model(h16):
    """The largest per-channel |mean| / sigma any InstanceNorm call of the small golden PredictionHead and PairUpdateWithMsa
    forwards receives (recorded; DESIGN.md states it next to the sweep)."""
    import numpy as np
    gold = os.path.join(os.path.dirname(__file__), "golden")
    seen = []
    real = ops.instnorm

    def spy(x, *a, **kw):
        v = x.double().reshape(x.shape[0], -1, x.shape[-1])
        seen.append((v.mean(1).abs() / v.std(1, unbiased=False).clamp_min(1e-300)).max().item())
        return real(x, *a, **kw)

    def load(name):
        z = np.load(os.path.join(gold, name + ".npz"), allow_pickle=False)
        Pw = {k[2:]: torch.from_numpy(z[k]).float() for k in z.files if k.startswith("w:")}
        I = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in:")}
        return Pw, {k: (v.float() if v.is_floating_point() else v).to(DEV) for k, v in I.items()}

    out = {}
    ops.instnorm = spy
    try:
        for name, make, call in (
                ("prediction_head", lambda: R.PredictionHead(8, 4, 0.0), lambda m, I: m(I["pair"])),
                ("c1_pair_update_with_msa", lambda: R.PairUpdateWithMsa(d_msa=96, d_proj=32, d_pair=64, n_heads=12, p_dropout=0.0),
                 lambda m, I: m(I["msa"], I["pair"], I["att"]))):
            Pw, I = load(name)
            m = make()
            m.load_state_dict(Pw, strict=True)
            del seen[:]
            call(m.to(DEV), I)
            torch.cuda.synchronize()
            assert seen, name
            out[name] = dict(calls=len(seen), max_mean_over_sigma=max(seen))
    finally:
        ops.instnorm = real
    INFO[f"instnorm_model/{dn(h16)}"] = out
    print("[rowops] instnorm in the model", dn(h16), out)


# ================================================================================================ softmax family
def run_softmax(name, rows, cols, h, *, y32, transposed, scale, spread, nbatch=0, ninf=False, seed=0):
    y_dt = F32 if y32 else h
    nb = max(nbatch, 1)
    x_rs, x_cs = (1, rows + 3) if transposed else (cols + 2, 1)
    x_bs = rows * cols + (rows + 3) * (cols + 2) + 5 if nbatch else 0
    y_rs = cols + 3
    y_bs = rows * y_rs + 7 if nbatch else 0
    xo = O.strided_offsets(O.PAD, (x_bs, x_rs, x_cs), (nb, rows, cols), DEV)
    vals = spread / 2 * O.randn((nb, rows, cols), seed, DEV) / f32abs(scale)
    if ninf and cols > 1:
        vals[nb - 1, rows - 1, cols // 2] = float("-inf")
    xs = O.image_storage(xo, vals, F32)
    yo = O.strided_offsets(O.PAD, (y_bs, y_rs, 1), (nb, rows, cols), DEV)
    y0 = O.out_storage(yo, y_dt)
    ys = y0.clone()
    if nbatch:
        ok(lib.rf_softmax_batched(P(xs, O.PAD), x_bs, x_rs, x_cs, P(ys, O.PAD), ops.dcode(y_dt), y_bs, y_rs, rows, cols, scale,
                                  nbatch, ops.stream()))
    else:
        ok(lib.rf_softmax(P(xs, O.PAD), x_rs, x_cs, P(ys, O.PAD), ops.dcode(y_dt), y_rs, rows, cols, scale, ops.stream()))
    torch.cuda.synchronize()
    O.assert_untouched(y0, ys, yo, what=name)
    a = (xs, O.PAD, x_bs, x_rs, x_cs, rows, cols, scale, nb)
    r64, r32 = O.both(O.softmax, y_dt, *a)
    got = ys[yo]
    O.compare(f"softmax/{name}/{dn(y_dt)}", got, r64, r32, O.softmax_allowance(O.softmax_logits(*a, dtype=F64)), exact=cols == 1)
    if ninf and cols > 1:
        assert got[nb - 1, rows - 1, cols // 2].item() == 0.0


def f32abs(v):
    return abs(O.f32(v))


@pytest.mark.parametrize("cols", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("rows", [1, 5, 9])
def test_softmax(h16, rows, cols):
    for i, (y32, tr, scale, spread, nbatch, ninf) in enumerate([
            (True, False, 1.0, 4, 0, False), (False, True, 0.17, 30, 0, True), (True, True, 1.0, 30, 3, True),
            (False, False, 0.17, 4, 3, False), (True, False, 0.17, 30, 0, True)]):
        run_softmax(f"{rows}x{cols}/tr{int(tr)}/s{scale}/spread{spread}/nb{nbatch}/inf{int(ninf)}", rows, cols, h16, y32=y32,
                    transposed=tr, scale=scale, spread=spread, nbatch=nbatch, ninf=ninf, seed=i)


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("L_", [5, 50, 65])
def test_tied_softmax(h16, L_, H):
    """att against the float64 softmax; the pad columns of rf_tied_softmax_ld exactly zero; the symmetrised map against the
    symmetrisation of the STORED att (a 16-bit att is symmetrised after its rounding: 0.5 * (a + b) of two stored values is
    one fp32 rounding, so that comparison is exact), bitwise symmetric."""
    B = 2
    lo = O.strided_offsets(O.PAD, (H * L_ * L_, L_ * L_, L_, 1), (B, H, L_, L_), DEV)
    ls = O.image_storage(lo, 3.0 * O.randn((B, H, L_, L_), L_ + H, DEV), F32)
    a = (ls, O.PAD, 0, L_, 1, B * H * L_, L_, 1.0, 1)
    extra = O.softmax_allowance(O.softmax_logits(*a, dtype=F64))
    for att_dt in (F32, h16):
        r64, r32 = O.both(O.softmax, att_dt, *a)
        for att_ld, sym_ld in ((L_, H), ((L_ + 8) // 8 * 8, H + 3)):
            ao = O.strided_offsets(O.PAD, (H * L_ * att_ld, L_ * att_ld, att_ld, 1), (B, H, L_, L_), DEV)
            zo = O.strided_offsets(O.PAD + L_, (att_ld, 1), (B * H * L_, att_ld - L_), DEV) if att_ld > L_ else None
            so = O.strided_offsets(O.PAD, (L_ * L_ * sym_ld, L_ * sym_ld, sym_ld, 1), (B, L_, L_, H), DEV)
            a0, s0 = O.out_storage(torch.cat([ao.reshape(-1), zo.reshape(-1)]) if zo is not None else ao, att_dt), O.out_storage(so, F32)
            as_, ss = a0.clone(), s0.clone()
            if att_ld == L_:
                ok(lib.rf_tied_softmax(P(ls, O.PAD), P(as_, O.PAD), ops.dcode(att_dt), P(ss, O.PAD), sym_ld, B, H, L_, ops.stream()))
            else:
                ok(lib.rf_tied_softmax_ld(P(ls, O.PAD), P(as_, O.PAD), ops.dcode(att_dt), att_ld, P(ss, O.PAD), sym_ld, B, H, L_,
                                          ops.stream()))
            torch.cuda.synchronize()
            O.assert_untouched(a0, as_, ao, zero_off=zo)
            O.assert_untouched(s0, ss, so)
            att = as_[ao]
            O.compare(f"tied_softmax/L{L_}/H{H}/ld{att_ld}/{dn(att_dt)}", att, r64.reshape(B, H, L_, L_), r32.reshape(B, H, L_, L_),
                      extra.reshape(B, H, L_, L_))
            sym = ss[so]
            s64 = O.tied_sym(att)
            O.compare(f"tied_softmax/sym/L{L_}/H{H}/ld{att_ld}/{dn(att_dt)}", sym, s64, O.rnd(s64, F32), exact=True)
            assert torch.equal(sym, sym.transpose(1, 2)), "sym is not bitwise symmetric"
    assert lib.rf_tied_softmax_ld(P(ls, O.PAD), P(as_, O.PAD), ops.dcode(h16), L_ + (4 if L_ % 8 != 4 else 2), None, 0, B, H, L_,
                                  ops.stream()) == EALIGN


POSWISE_ROUTES = {  # name: (k / q_scale 16-bit?, q0 16-bit?, dlen, k_col0)
    "h16xh16": (True, True, 16, 8), "f32xh16": (True, False, 16, 8), "f32xf32": (False, False, 16, 8),
    "scalar-dlen12": (True, True, 12, 8), "scalar-offset": (True, True, 16, 3), "scalar-f32-offset": (False, False, 16, 3)}


@pytest.mark.parametrize("N,H", [(1, 1), (5, 12), (70, 1), (130, 12)])
@pytest.mark.parametrize("route", list(POSWISE_ROUTES))
def test_poswise(h16, route, N, H):
    """the three vector dot products and the scalar one (dlen = 12, or a column offset off the vector alignment), with w only,
    the in-place q scaling only (vector for an aligned 16-bit q, scalar otherwise) and both"""
    k16, q16, dlen, col0 = POSWISE_ROUTES[route]
    k_dt, q_dt = (h16 if k16 else F32), (h16 if q16 else F32)
    B, L_ = 2, 3
    q0_ld, k_ld, k_hs, qs_ld, qs_dh = H * dlen + 8, col0 + H * dlen + 8, dlen, col0 + H * dlen + 16, dlen
    scale, qscale = dlen ** -0.5, 0.3
    qo = O.strided_offsets(O.PAD, (L_ * q0_ld, q0_ld, dlen, 1), (B, L_, H, dlen), DEV)
    ko = O.strided_offsets(O.PAD + col0, (N * L_ * k_ld, L_ * k_ld, k_ld, k_hs, 1), (B, N, L_, H, dlen), DEV)
    q0s = O.image_storage(qo, O.randn(tuple(qo.shape), N + H, DEV), q_dt)
    ks = O.image_storage(ko, 1.5 * O.randn(tuple(ko.shape), N + H + 1, DEV), k_dt)
    a = (q0s, O.PAD, q0_ld, ks, O.PAD, k_ld, col0, k_hs, dlen, B, N, L_, H, scale)
    w64, w32 = O.both(O.poswise, F32, *a)
    wx = O.softmax_allowance(O.poswise_logits(*a, dtype=F64)).permute(0, 3, 2, 1)  # [B, N, H, L]
    so = O.strided_offsets(O.PAD + col0, (N * L_ * qs_ld, L_ * qs_ld, qs_ld, qs_dh, 1), (B, N, L_, H, qs_dh), DEV)
    qv = O.randn(tuple(so.shape), N + H + 2, DEV).to(k_dt)
    wo = O.strided_offsets(O.PAD, (N * H * L_, H * L_, L_, 1), (B, N, H, L_), DEV)
    for want_w, want_qs in ((True, False), (False, True), (True, True)):
        w0 = O.out_storage(wo, F32)
        wst = w0.clone()
        q0 = O.out_storage(so, k_dt)
        q0[so.reshape(-1)] = qv.reshape(-1)
        qst = q0.clone()
        ok(lib.rf_poswise(P(q0s, O.PAD), ops.dcode(q_dt), q0_ld, P(ks, O.PAD), k_ld, col0, k_hs, dlen, P(wst, O.PAD) if want_w else None,
                          P(qst, O.PAD) if want_qs else None, qs_ld, col0, qs_dh, ops.dcode(k_dt), B, N, L_, H, scale, qscale, ops.stream()))
        torch.cuda.synchronize()
        O.assert_untouched(w0, wst, wo if want_w else wo[:0])
        O.assert_untouched(q0, qst, so if want_qs else so[:0])
        nm = f"poswise/{route}/N{N}/H{H}/w{int(want_w)}q{int(want_qs)}"
        if want_w:  # compared in [B, L, H, N]: a row is one softmax
            O.compare(nm + "/w", wst[wo].permute(0, 3, 2, 1), w64.permute(0, 3, 2, 1), w32.permute(0, 3, 2, 1), wx.permute(0, 3, 2, 1),
                      exact=N == 1)
        if want_qs:
            s64, s32 = (O.poswise_qscale(qv, w64, qscale, dtype=F64), O.rnd(O.poswise_qscale(qv, w64.float(), qscale, dtype=F32), k_dt))
            sx = (qv.double() * O.f32(qscale)).abs() * wx.permute(0, 1, 3, 2)[..., None]
            O.compare(nm + "/qs", qst[so].reshape(-1, H * qs_dh), s64.reshape(-1, H * qs_dh), s32.reshape(-1, H * qs_dh),
                      sx.reshape(-1, H * qs_dh))


def test_poswise_refuses_more_logits_than_lds(h16):
    t = torch.zeros(64, device=DEV)
    assert lib.rf_poswise(P(t), 0, 16, P(t), 16, 0, 16, 16, P(t), None, 0, 0, 0, 0, 1, 16385 // 12 + 1, 1, 12, 1.0, 1.0, ops.stream()) == EINVAL


@pytest.mark.parametrize("D", [1, 288, 300])
@pytest.mark.parametrize("N", [1, 37])
def test_weighted_msa_sum(h16, N, D):
    B, L_, y_ld = 2, 3, D + 5
    xo = O.row_offsets(O.PAD, D, B * N * L_, D, DEV)
    wo = O.row_offsets(O.PAD, L_, B * N, L_, DEV)
    ws = O.image_storage(wo, torch.softmax(O.randn((B, N, L_), N + D, DEV), 1), F32)
    yo = O.row_offsets(O.PAD, y_ld, B * L_, D, DEV)
    for x_dt in (F32, h16):
        xs = O.image_storage(xo, O.randn((B * N * L_, D), N + D + 1, DEV) + 2.0, x_dt)
        y0 = O.out_storage(yo, F32)
        ys = y0.clone()
        ok(lib.rf_weighted_msa_sum(P(xs, O.PAD), ops.dcode(x_dt), P(ws, O.PAD), P(ys, O.PAD), y_ld, B, N, L_, D, ops.stream()))
        torch.cuda.synchronize()
        O.assert_untouched(y0, ys, yo)
        r64, r32 = O.both(O.weighted_msa_sum, F32, xs, O.PAD, ws, O.PAD, B, N, L_, D)
        # N = 1: the one weight is softmax of one logit, exactly 1, and the sum is a copy
        O.compare(f"weighted_msa_sum/N{N}/D{D}/{dn(x_dt)}", ys[yo], r64.reshape(B * L_, D), r32.reshape(B * L_, D), exact=N == 1)


@pytest.mark.parametrize("n", [5, 64, 130])
@pytest.mark.parametrize("transposed", [0, 1])
@pytest.mark.parametrize("is_query", [0, 1])
def test_favor_softmax_features(h16, is_query, transposed, n):
    S, n1, n2, m, m_pad, dh, eps = 4, 1, 2, 266, 288, 64, 1e-4
    xstr = (2 * n2 * n * 3 * dh + 11, 0, n * 3 * dh + 5, 3 * dh)  # rows of a packed q | k | v buffer
    s = O.ar(S, DEV)
    xb = (s // (n2 * n1)) * xstr[0] + ((s // n2) % n1) * xstr[1] + (s % n2) * xstr[2]
    xo = O.PAD + dh + xb[:, None, None] + O.ar(n, DEV)[None, :, None] * xstr[3] + O.ar(dh, DEV)
    do = O.favor_offsets(O.PAD, S, n, m_pad, transposed, DEV)
    for dt in (F32, h16):
        xs = O.image_storage(xo, 0.6 * O.randn((S, n, dh), n, DEV), dt)
        ds = O.image_storage(do[..., :m], 1.5 * O.randn((S, n, m), n + 1, DEV), dt)
        ds = torch.cat([ds, torch.full((do.max().item() + 1 + O.PAD - ds.numel(),), float("nan"), device=DEV, dtype=dt)])
        y0 = O.out_storage(do, dt)
        ys = y0.clone()
        ok(lib.rf_favor_softmax_features(P(ds, O.PAD), P(xs, O.PAD + dh), ops._i4(xstr), n1, n2, P(ys, O.PAD), ops.dcode(dt), S, n, m, m_pad,
                                         dh, is_query, transposed, eps, ops.stream()))
        torch.cuda.synchronize()
        O.assert_untouched(y0, ys, do)
        a = (ds, O.PAD, xs, O.PAD + dh, xstr, n1, n2, S, n, m, m_pad, dh, is_query, transposed)
        r64 = O.favor_features(*a, eps=eps, dtype=F64)
        r32 = O.rnd(O.favor_features(*a, eps=eps, dtype=F32), dt)
        extra = torch.nn.functional.pad(float(m) ** -0.5 * O.exp_allowance(O.favor_exponent(*a, dtype=F64)), (0, m_pad - m))
        got = ys[do]
        O.compare(f"favor_features/q{is_query}/t{transposed}/n{n}/{dn(dt)}", got, r64, r32, extra)
        assert (got[..., m:] == 0).all() and not torch.signbit(got[..., m:]).any(), "pad features are not exactly zero"


def test_linattn_normalize(h16):
    rows, dh, num_ld, y_ld = 37, 64, 64 + 1 + 3, 64 + 5
    no = O.row_offsets(O.PAD, num_ld, rows, dh + 1, DEV)
    vals = O.randn((rows, dh + 1), 3, DEV)
    vals[:, dh] = vals[:, dh].abs() + 0.5
    ns = O.image_storage(no, vals, F32)
    yo = O.row_offsets(O.PAD, y_ld, rows, dh, DEV)
    for y_dt in (F32, h16):
        y0 = O.out_storage(yo, y_dt)
        ys = y0.clone()
        ok(lib.rf_linattn_normalize(P(ns, O.PAD), num_ld, P(ys, O.PAD), ops.dcode(y_dt), y_ld, rows, dh, ops.stream()))
        torch.cuda.synchronize()
        O.assert_untouched(y0, ys, yo)
        r64, r32 = O.both(O.linattn_normalize, y_dt, ns, O.PAD, num_ld, rows, dh)
        O.compare(f"linattn_normalize/{dn(y_dt)}", ys[yo], r64, r32)


# ================================================================================================ element-wise
def run_axpby(name, n, h, x16, z16, y16, *, route, mis=0, with_z=True, inplace=False, a=0.7153, b=-1.3291, seed=0):
    x_dt, z_dt, y_dt = (h if x16 else F32), (h if z16 else F32), (h if y16 else F32)
    off = O.PAD + mis
    o = off + O.ar(n, DEV)
    xs = O.image_storage(o, O.randn((n,), seed, DEV), x_dt)
    zs = O.image_storage(o, O.randn((n,), seed + 1, DEV), z_dt) if with_z else None
    r64, r32 = O.both(O.axpby, y_dt, xs[o], a, zs[o] if with_z else None, b)
    if inplace:
        assert x_dt == y_dt
        y0, ys = xs.clone(), xs
    else:
        y0 = O.out_storage(o, y_dt)
        ys = y0.clone()
    ok(lib.rf_axpby(P(xs, off), ops.dcode(x_dt), a, P(zs, off) if with_z else None, ops.dcode(z_dt) if with_z else 0, b, P(ys, off),
                    ops.dcode(y_dt), n, ops.stream()))
    assert lib.rf_rowops_last_route() == route, (name, lib.rf_rowops_last_route())
    torch.cuda.synchronize()
    O.assert_untouched(y0, ys, o, what=name)
    W = next((w for w in (100, 16, 4) if n % w == 0), n)  # rows of the comparison: short, or the whole vector when n is ragged
    exact = a == 1.0 and not with_z  # a conversion
    O.compare(f"axpby/{name}/{dn(x_dt)},{dn(z_dt) if with_z else '-'}->{dn(y_dt)}", ys[o].reshape(-1, W), r64.reshape(-1, W),
              r32.reshape(-1, W), exact=exact, route=O.ROUTES[route])


@pytest.mark.parametrize("x16,z16,y16", [(x, z, y) for x in (0, 1) for z in (0, 1) for y in (0, 1)])
def test_axpby(h16, x16, z16, y16):
    """n4 = 1: no thread has a second group; 300: threads 0..43 of the one workgroup do; 700: two workgroups, stride 512,
    threads 0..187 do.  Scalar route by n % 4 and by a pointer one element off."""
    for n4 in (1, 300, 700):
        run_axpby(f"vec-n4_{n4}", 4 * n4, h16, x16, z16, y16, route=41, seed=n4)
    run_axpby("scalar-tail", 4 * 300 + 1, h16, x16, z16, y16, route=40)
    run_axpby("scalar-offset", 4 * 300, h16, x16, z16, y16, route=40, mis=1)
    run_axpby("vec-noz", 4 * 300, h16, x16, z16, y16, route=41, with_z=False)
    run_axpby("vec-convert", 4 * 700, h16, x16, z16, y16, route=41, with_z=False, a=1.0)
    run_axpby("scalar-convert", 4 * 700 + 3, h16, x16, z16, y16, route=40, with_z=False, a=1.0)
    if x16 == y16:
        run_axpby("vec-inplace", 4 * 700, h16, x16, z16, y16, route=41, inplace=True)
        run_axpby("scalar-inplace", 4 * 300 + 2, h16, x16, z16, y16, route=40, inplace=True)


def test_axpby_grid_loop():
    """n4 = 16384 * 512 + 300 above the grid cap of 16384 workgroups: the two-group loop takes a second, partial pass"""
    R.set_compute_dtype(torch.bfloat16)
    run_axpby("vec-loop", 4 * (16384 * 512 + 300), torch.bfloat16, 1, 1, 1, route=41)


def test_copy4d(h16):
    dims = (2, 3, 5, 7)
    n = 2 * 3 * 5 * 7
    for x_dt, y_dt in ((F32, h16), (h16, F32), (F32, F32), (h16, h16)):
        for xs_, ys_ in (((7, 70, 14, 1), (105, 35, 7, 1)),      # a permuted, gapped source into a dense destination
                         ((105, 35, 7, 1), (8, 16, 48, 240))):    # a dense source into a fully permuted, gapped destination
            xo, yo = O.strided_offsets(O.PAD + 1, xs_, dims, DEV), O.strided_offsets(O.PAD + 3, ys_, dims, DEV)
            xs = O.image_storage(xo, O.randn(dims, n, DEV), x_dt)
            y0 = O.out_storage(yo, y_dt)
            ys = y0.clone()
            ok(lib.rf_copy4d(P(xs, O.PAD + 1), ops.dcode(x_dt), ops._i4(xs_), P(ys, O.PAD + 3), ops.dcode(y_dt), ops._i4(ys_), ops._i4(dims),
                             ops.stream()))
            torch.cuda.synchronize()
            O.assert_untouched(y0, ys, yo)
            r64 = xs[xo].double()
            O.compare(f"copy4d/{dn(x_dt)}->{dn(y_dt)}/{xs_}->{ys_}", ys[yo], r64, O.rnd(r64, y_dt), exact=True)


def test_scale_rows(h16):
    rows, D = 37, 72
    o = O.row_offsets(O.PAD, D, rows, D, DEV)
    w = O.randn((rows,), 5, DEV).float()
    for dt in (F32, h16):
        xs = O.image_storage(o, O.randn((rows, D), 6, DEV), dt)
        y0 = O.out_storage(o, dt)
        ys = y0.clone()
        ok(lib.rf_scale_rows(P(xs, O.PAD), P(ys, O.PAD), ops.dcode(dt), P(w), rows, D, ops.stream()))
        torch.cuda.synchronize()
        O.assert_untouched(y0, ys, o)
        r64, r32 = O.both(O.scale_rows, dt, xs[o], w)
        # fp32: one multiplication, the float64 product rounded once; 16-bit: fp32 product rounded again (inside the bound)
        O.compare(f"scale_rows/{dn(dt)}", ys[o], r64, r32, exact=dt == F32)
        x0 = xs.clone()
        ok(lib.rf_scale_rows(P(xs, O.PAD), P(xs, O.PAD), ops.dcode(dt), P(w), rows, D, ops.stream()))  # in place
        torch.cuda.synchronize()
        O.assert_untouched(x0, xs, o)
        assert torch.equal(xs[o], ys[o])


@pytest.mark.parametrize("P2,c0,ld,route", [(6, 2, 17, 42), (8, 4, 24, 43), (8, 4, 22, 42), (8, 2, 24, 42)])
def test_tile_1d_feats(h16, P2, c0, ld, route):
    B, L_ = 2, 5
    m1 = O.randn((B * L_ * P2,), P2, DEV).float()
    ms = torch.cat([torch.full((4,), float("nan"), device=DEV), m1, torch.full((4,), float("nan"), device=DEV)])
    fo = O.row_offsets(O.PAD + c0, ld, B * L_ * L_, 2 * P2, DEV)
    for dt in (F32, h16):
        f0 = O.out_storage(fo, dt)
        fs = f0.clone()
        ok(lib.rf_tile_1d_feats(P(ms, 4), P(fs, O.PAD), ops.dcode(dt), ld, c0, B, L_, P2, ops.stream()))
        assert lib.rf_rowops_last_route() == route
        torch.cuda.synchronize()
        O.assert_untouched(f0, fs, fo)
        r64 = O.tile_1d_feats(m1, B, L_, P2).reshape(B * L_ * L_, 2 * P2)
        O.compare(f"tile_1d_feats/P{P2}/c{c0}/ld{ld}/{dn(dt)}", fs[fo], r64, O.rnd(r64, dt), exact=True, route=O.ROUTES[route])


# ================================================================================================ the route table
def test_every_route_code_is_reached(h16):
    """One small case per code of rf_rowops_last_route (each asserts its code and goes through the same comparison), and the
    table in include/rfmi.h lists exactly these codes."""
    h = h16
    witness = {
        1: lambda: run_ln("w", 9, 288, h, route=1), 2: lambda: run_ln("w", 9, 384, h, route=2),
        3: lambda: run_sym(288, 3, 0, 3, h, True), 4: lambda: run_sym(384, 4, 0, 3, h, True),
        5: lambda: run_ln("w", 3, 256, h, route=5), 6: lambda: run_ln("w", 3, 768, h, route=6),
        7: lambda: run_ln("w", 3, 768, h, route=7, x16=True), 8: lambda: run_ln("w", 9, 32, h, route=8),
        9: lambda: run_ln("w", 9, 64, h, route=9),
        30: lambda: run_instnorm("w", 1, 130, 20, h, x16=False, routes=(30, 32)),
        31: lambda: run_instnorm("w", 1, 130, 16, h, x16=True, routes=(31, 33)),
        32: lambda: run_instnorm("w", 1, 130, 16, h, x16=True, centre=True, routes=(31, 32)),
        33: lambda: run_instnorm("w", 1, 600, 72, h, x16=True, routes=(31, 33)),
        34: lambda: run_instnorm("w", 1, 9, 72, h, x16=True, routes=(31, 34)),
        40: lambda: run_axpby("w", 7, h, 0, 0, 0, route=40), 41: lambda: run_axpby("w", 8, h, 0, 0, 0, route=41),
        42: lambda: test_tile_1d_feats(h, 6, 2, 17, 42), 43: lambda: test_tile_1d_feats(h, 8, 4, 24, 43),
    }
    for i, D in enumerate((40, 100, 200, 352, 500, 1000, 1100)):
        witness[10 + i] = lambda D=D, i=i: run_ln("w", 5, D + 1, h, route=10 + i)
        witness[20 + i] = lambda D=D, i=i: run_sym(D, 20 + i, 0, 2, h, True)
    assert sorted(witness) == sorted(O.ROUTES)
    for code in sorted(witness):
        witness[code]()
        # (the InstanceNorm witnesses leave the apply kernel's code: 30 / 31 are asserted inside run_instnorm after the statistics)
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rfmi.h")).read()
    table = hdr[hdr.index("Introspection for tests and measurement tools"):hdr.index("int rf_rowops_last_route")]
    listed = set()
    for a, sep, b in re.findall(r"^ \*\s+(\d+)(?: (/|\.\.) (\d+))?  ", table, flags=re.M):
        listed |= set(range(int(a), int(b) + 1)) if sep == ".." else ({int(a), int(b)} if sep else {int(a)})
    assert listed == set(O.ROUTES), sorted(listed ^ set(O.ROUTES))
