"""tests/grad_oracle.py checked without a GPU: the row cuts of `errors` against a case worked out by hand, the exact-zero rule,
`held` and `compare` on planted results either side of their ceilings (a rule must not reject a correct gradient and must reject
a wrong one), and `oracle_grads` on a two-layer ReLU toy: the order of the jitter's draws against a loop written out here, the
inputs and parameters that are set apart, and a planted kink that lifts a floor above the ceiling."""
import math

import pytest
import torch
import torch.nn.functional as F

import grad_oracle as G

F64 = torch.float64
BF16 = torch.bfloat16


# ------------------------------------------------------------------------------------------------ errors
def hand_case():
    """want [B=1, N=2, L=2, C=2] with one zero (n, l) row; got differs in three elements"""
    want = torch.tensor([[[[3.0, 4.0], [0.0, 0.0]], [[0.0, 5.0], [12.0, 0.0]]]], dtype=F64)
    got = want.clone()
    got[0, 0, 0, 0] += 1
    got[0, 1, 1, 0] += 2
    got[0, 1, 0, 1] += 3
    return got, want


def test_errors_row_cuts_against_a_hand_computed_case():
    got, want = hand_case()
    whole = math.sqrt(14) / math.sqrt(194)
    # the last dimension: rows [3,4] [0,0] [0,5] [12,0]; the trailing two: one per n; "bl": every n of one l
    for rows, worst in ((1, 3 / 5), (2, math.sqrt(13) / 13), ("bl", math.sqrt(10) / math.sqrt(50))):
        a, r = G.errors(got, want, rows)
        assert a == pytest.approx(whole, rel=1e-14) and r == pytest.approx(worst, rel=1e-14), rows
    a, r = G.errors(got[0, :, 0], want[0, :, 0], "bl")     # [B, L, C]: a row is one (b, l)
    assert r == pytest.approx(3 / 5, rel=1e-14)
    assert G.errors(want, want, 1) == (0.0, 0.0)


def test_errors_zero_row_and_zero_tensor_are_infinite():
    got, want = hand_case()
    got[0, 0, 1, 1] = 1e-30                                   # the zero row of `want`
    a, r = G.errors(got, want, 1)
    assert math.isfinite(a) and r == float("inf")
    assert G.errors(got, want, 2)[1] < 1                      # (as part of a longer row it is an ordinary error)
    zero = torch.zeros(2, 3, dtype=F64)
    assert G.errors(zero, zero) == (0.0, 0.0)
    off = zero.clone()
    off[1, 2] = 1e-30
    assert G.errors(off, zero) == (float("inf"), float("inf"))
    with pytest.raises(AssertionError):
        G.errors(torch.full((2, 3), float("nan")), zero)


# ------------------------------------------------------------------------------------------------ held
def test_held_either_side_of_the_ceiling():
    want = torch.randn(3, 5, 7, generator=G.gen(1), dtype=F64)
    y, unit = 1e-5, 2.0 ** -24
    ref32 = want * (1 + y)                                    # the same relative error in the whole tensor and in every row
    ceiling = G.MARGIN * y
    records = []
    call = lambda got, **kw: G.held({"dx": got}, {"dx": want}, {"dx": ref32}, "case", unit, 1, records, **kw)  # noqa: E731
    assert call(want * (1 + 0.5 * ceiling))
    assert not call(want * (1 + 2 * ceiling))
    worse = want.clone()
    worse[1, 2] *= 1 + 2 * ceiling                            # one row alone: the whole tensor passes, the worst row does not
    assert G.errors(worse, want)[0] < ceiling and not call(worse, key="out")
    assert [r["case"] for r in records] == ["case"] * 3
    assert all(r["grad"] == "dx" for r in records[:2]) and records[2]["out"] == "dx" and "grad" not in records[2]
    rec = records[0]
    assert rec["ceiling_rel_l2"] == pytest.approx(ceiling, rel=1e-6) and rec["ceiling_worst_row"] == pytest.approx(ceiling, rel=1e-6)
    assert rec["rel_l2"] == pytest.approx(0.5 * ceiling, rel=1e-6) and rec["f32_autograd_rel_l2"] == pytest.approx(y, rel=1e-6)
    assert set(rec) == {"case", "grad", "rel_l2", "worst_row", "f32_autograd_rel_l2", "f32_autograd_worst_row", "unit",
                        "ceiling_rel_l2", "ceiling_worst_row"}


def test_held_unit_takes_over_when_float32_autograd_is_exact():
    want = torch.randn(4, 6, generator=G.gen(2), dtype=F64)
    units = {"a": 2.0 ** -24, "b": 2.0 ** -8}
    ref = {"a": want, "b": want}
    records = []
    good = {"a": want * (1 + 2 * units["a"]), "b": want * (1 + 2 * units["b"])}
    assert G.held(good, ref, ref, "t", units, {"a": 1, "b": 2}, records)
    assert [r["ceiling_rel_l2"] for r in records] == [4 * units["a"], 4 * units["b"]]
    assert all(r["f32_autograd_rel_l2"] == 0.0 for r in records)
    bad = dict(good, a=want * (1 + 8 * units["a"]))           # fine under b's unit, not under its own
    assert not G.held(bad, ref, ref, "t", units, 1, records)


# ------------------------------------------------------------------------------------------------ oracle_grads
def toy(P, x, c):
    """two layers with a ReLU between them; `m.proj` mixes the input (a buffer: no gradient), c scales the output"""
    h = F.relu(F.linear(x @ P["m.proj"], P["m.l1.weight"], P["m.l1.bias"]))
    return F.linear(h, P["m.l2.weight"]) * c


def toy_case(plant=False):
    g = G.gen(7)
    P = {"m.l1.weight": torch.randn(6, 4, generator=g, dtype=F64), "m.proj": torch.randn(4, 4, generator=g, dtype=F64),
         "m.l1.bias": torch.randn(6, generator=g, dtype=F64), "m.unused": torch.randn(3, generator=g, dtype=F64),
         "m.l2.weight": torch.randn(5, 6, generator=g, dtype=F64)}
    x, c = torch.randn(1, 4, generator=g, dtype=F64), torch.rand(1, 5, generator=g, dtype=F64) + 0.5
    z = F.linear(x @ P["m.proj"], P["m.l1.weight"])
    # pre-activations of +-1 and +-2 (every unit well away from the kink), or four of them within 1e-3 rounding units of it
    target = torch.tensor([1.0, -1.0, 2.0, -2.0, 1.0, -1.0], dtype=F64)
    if plant:
        target[:4] = torch.tensor([1.0, -1.0, 1.0, -1.0], dtype=F64) * 1e-3 * G.UNIT[BF16] * z[0, :4].abs()
    P["m.l1.bias"] = target - z[0]
    return P, {"x": x, "c": c}, torch.randn(1, 5, generator=g, dtype=F64)


def test_oracle_grads_draws_in_the_documented_order():
    P, inputs, w = toy_case()
    seen = []

    def fn(P_, x, c):
        seen.append((P_, x, c))
        return toy(P_, x, c)
    unit, seed = G.UNIT[BF16], 3
    ref, floor = G.oracle_grads(fn, P, inputs, w, unit, seed, fixed=("c",), frozen=("m.proj",))
    assert set(ref) == {"m.l1.weight", "m.l1.bias", "m.l2.weight", "x", "c"} == set(floor)     # m.unused: absent; m.proj: frozen
    plain, jittered = seen
    assert torch.equal(jittered[2], inputs["c"]) and torch.equal(plain[2], inputs["c"])       # a fixed input is never jittered
    assert not jittered[0]["m.proj"].requires_grad and not plain[0]["m.proj"].requires_grad
    # the loop, written out: parameters in dict order (the frozen one in its turn), then the inputs that are not fixed
    g = G.gen(seed + 1000)
    jit = lambda t: t * (1 + unit * (2 * torch.rand(t.shape, generator=g, dtype=F64) - 1))  # noqa: E731
    Pj = {k: jit(v).requires_grad_(k != "m.proj") for k, v in P.items()}
    xj, cj = jit(inputs["x"]).requires_grad_(), inputs["c"].clone().requires_grad_()
    for k in P:
        assert torch.equal(jittered[0][k], Pj[k].detach()), k
    assert torch.equal(jittered[1], xj.detach())
    (toy(Pj, xj, cj) * w).sum().backward()
    want = {**{k: Pj[k].grad for k in ("m.l1.weight", "m.l1.bias", "m.l2.weight")}, "x": xj.grad, "c": cj.grad}
    for k in ref:
        assert floor[k] == G.rel(want[k], ref[k]), k
    # marking c as fixed moved nobody else's draws: without it x is drawn the same, and c after it
    seen.clear()
    G.oracle_grads(fn, P, inputs, w, unit, seed, frozen=("m.proj",))
    assert torch.equal(seen[1][1], xj.detach()) and not torch.equal(seen[1][2], inputs["c"])
    # and without a unit there is one run and no floor
    seen.clear()
    again, none = G.oracle_grads(fn, P, inputs, w, frozen=("m.proj",))
    assert none is None and len(seen) == 1 and all(torch.equal(again[k], ref[k]) for k in ref)


def test_oracle_grads_missing_and_callable_loss():
    P, inputs, w = toy_case()
    absent, _ = G.oracle_grads(toy, P, inputs, w, frozen=("m.proj",))
    zeros, floor = G.oracle_grads(toy, P, inputs, w, G.UNIT[BF16], frozen=("m.proj",), missing="zeros")
    assert "m.unused" not in absent and "m.proj" not in absent and "m.proj" not in zeros
    assert torch.equal(zeros["m.unused"], torch.zeros(3, dtype=F64)) and floor["m.unused"] == 0.0
    assert all(torch.equal(absent[k], zeros[k]) for k in absent)
    twice, _ = G.oracle_grads(lambda P_, x, c: (toy(P_, x, c), toy(P_, x, c)), P, inputs, lambda o: ((o[0] + o[1]) * w).sum(),
                              frozen=("m.proj",))
    assert all(torch.allclose(twice[k], 2 * absent[k], rtol=1e-14, atol=0) for k in absent)
    with pytest.raises(AssertionError):
        G.oracle_grads(toy, P, inputs, w, missing="none")


def test_a_planted_kink_lifts_the_floor_above_the_ceiling():
    for plant in (False, True):
        P, inputs, w = toy_case(plant)
        _, floor = G.oracle_grads(toy, P, inputs, w, G.UNIT[BF16], fixed=("c",), frozen=("m.proj",))
        for key in ("m.l1.weight", "m.l1.bias", "x"):          # what sits in front of the ReLU
            assert (floor[key] > G.CEIL[BF16]) == plant, (plant, key, floor[key])
            assert (G.tolerance(BF16, floor, key) == G.CEIL[BF16]) != plant
    assert G.tolerance(BF16, None, "x") == G.CEIL[BF16]


# ------------------------------------------------------------------------------------------------ compare
def test_compare_rejects_and_names_a_gradient_at_twice_its_tolerance(capsys):
    g = G.gen(4)
    ref = {k: torch.randn(8, 3, generator=g, dtype=F64) for k in ("a", "b", "c")}
    floor = {"a": 0.0, "b": 1e-2, "c": 0.0}                   # b's tolerance is 3e-2, the others' 1e-2
    near = {"a": ref["a"] * (1 + 0.5e-2), "b": ref["b"] * (1 + 2e-2), "c": ref["c"]}
    G.compare(near, ref, torch.float16, "toy", floor)
    out = capsys.readouterr().out
    assert out.count("\n") == 3 and "toy b: rel-L2 2.000e-02 (tolerance 3.000e-02, kink floor 1.000e-02)" in out
    with pytest.raises(AssertionError) as exc:
        G.compare(dict(near, b=ref["b"] * (1 + 6e-2), c=ref["c"] * (1 + 2e-2)), ref, torch.float16, "toy", floor)
    assert "'b'" in str(exc.value) and "'c'" in str(exc.value) and "'a'" not in str(exc.value)
    with pytest.raises(AssertionError):                        # strict: a gradient at its tolerance is rejected
        G.compare({"a": ref["a"] * 3}, {"a": ref["a"] * 2}, torch.float16, "toy", {"a": 0.5 / 3})
    with pytest.raises(AssertionError):                        # without floors the ceiling alone holds
        G.compare(near, ref, torch.float16, "toy")
    with pytest.raises(AssertionError):                        # a gradient the reference has and the module lacks
        G.compare({"a": ref["a"]}, ref, torch.float16, "toy", floor)


def test_compare_exact_zero_arguments():
    g = G.gen(5)
    ref = {"w": torch.randn(4, 4, generator=g, dtype=F64), "bias": torch.randn(4, generator=g, dtype=F64) * 1e-18}
    got = {"w": ref["w"].clone(), "bias": torch.zeros(4), "far": torch.zeros(2)}
    bound = {"bias": 1e-9 * ref["w"].norm()}
    G.compare(got, ref, torch.float32, "toy", zero=bound, unreached_zero=True)
    one = torch.zeros(4)
    one[2] = 1e-30
    with pytest.raises(AssertionError):                        # an "exact zero" with one non-zero element
        G.compare(dict(got, bias=one), ref, torch.float32, "toy", zero=bound)
    with pytest.raises(AssertionError):                        # the oracle's own value is no rounding noise
        G.compare(got, dict(ref, bias=ref["bias"] * 1e12), torch.float32, "toy", zero=bound)
    with pytest.raises(AssertionError):                        # a parameter the loss does not reach
        G.compare(dict(got, far=torch.tensor([0.0, 1e-30])), ref, torch.float32, "toy", zero=bound, unreached_zero=True)
    G.compare(dict(got, far=torch.ones(2)), ref, torch.float32, "toy", zero=bound)    # (not asked for: the call site's business)
    # norms: the error against the size the call site gives, the oracle's noise against 1e-10 of it
    size = ref["w"].norm().item()
    G.compare(dict(got, bias=torch.full((4,), 1e-5 * size / 2)), ref, torch.float32, "toy", norms={"bias": size})
    with pytest.raises(AssertionError):
        G.compare(dict(got, bias=torch.full((4,), 1e-4 * size)), ref, torch.float32, "toy", norms={"bias": size})
    with pytest.raises(AssertionError):
        G.compare(got, dict(ref, bias=ref["bias"] * 1e12), torch.float32, "toy", norms={"bias": size})
