"""The two rules every gradient test holds a HIP backward pass to, and the helpers those tests share.  Importing this module
needs neither a GPU nor the built libraries (tests/test_grad_oracle_cpu.py plants defects and shows that the rules reject them).

The yardstick rule -- a kernel against float64 autograd (`errors`, `held`).  The reference is float64 autograd of a restatement
of the forward on the operands as the kernel reads them (already rounded to their storage type).  The ceiling of an output is
not fixed in advance: it is MARGIN = 4 times a yardstick measured at run time, the larger of (a) the error of torch's own float32
autograd of the same restatement on the same operands against the float64 result and (b) the rounding unit of the output's
storage type (UNIT: 2^-24 for fp32, 2^-11 for fp16, 2^-8 for bf16).  Both the relative L2 error of the whole tensor and that of
the worst row are held, each to its own yardstick, with `<=`; the margin is 4 because a row of two or three terms averages no
rounding error away.  What a row is belongs to the kernel (one softmax, one (b, i) of an attention map, one table row) and is
the `rows` argument: an int k for the trailing k dimensions, or "bl" for everything of one (b, l) of a [B, L, ..] or
[B, N, L, ..] tensor.  A row, or a whole tensor, that is exactly zero in float64 must be exactly zero: anything else there is an
infinite error.

The ceiling-or-kink-floor rule -- a module against the CPU oracle (`oracle_grads`, `tolerance`, `compare`).  The reference is
float64 autograd through oracle/rf_oracle.py (or a restatement with the dropouts' keep maps) of sum(module(...) * w) for a random
w.  The relative L2 error of each whole gradient is held, with a strict `<`, to max(CEIL[mode], 3 x kink floor): CEIL is the
project's standing ceiling (1e-4 fp32, 1e-2 fp16, 5e-2 bf16).  A ReLU or ELU makes the exact gradient a discontinuous function of
the forward's values: wherever a pre-activation lies within rounding distance of 0 the forward of a mode may take the other side
of the kink.  The kink floor of a gradient is the float64 gradient's own relative change under a relative jitter of one rounding
unit of the mode (UNIT) on every parameter and every input, drawn from gen(seed + 1000) for the parameters in dict order and then
for the inputs in call order.  `fixed` inputs (coordinates that enter through a distance mask alone) are not jittered and take
no draws.  `frozen` parameters (a buffer the state dict carries, such as a random projection) get no gradient; a mode rounds
them like any other operand, so they are jittered in their turn.  A function without kinks is held to CEIL alone (no `unit`).
Gradients whose exact value is zero have no relative error; the call site names them: `zero` (a bias that moves a whole
softmax row: exactly zero here, and the oracle's own value below the noise bound the call site gives), `norms` (a sum of terms
that cancel: the error and the oracle's own 1e-10 noise bound are taken against the size the call site gives, under CEIL) and
`unreached_zero` (parameters the loss does not reach have no gradient in the oracle and exact zeros here)."""
import contextlib
import json
import os

import pytest
import torch

DEV = "cuda"
MODES = [torch.float32, torch.bfloat16, torch.float16]
MODE_IDS = ["fp32", "bf16", "fp16"]
CEIL = {torch.float32: 1e-4, torch.float16: 1e-2, torch.bfloat16: 5e-2}
UNIT = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
MARGIN = 4.0


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rel(a, b):
    """relative L2 error of a against b, in float64 on the CPU"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def state(mod, pre="m"):
    return {f"{pre}.{k}": v.detach().double().cpu() for k, v in mod.state_dict().items()}


def randomize(mod, seed, centred):
    """non-trivial biases and norm affines (the defaults 0 / 1 would hide their gradients' mistakes): every 1-D parameter is drawn
    at a scale of 0.1, around 1 where centred(name) says so, around 0 elsewhere"""
    g = gen(seed)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if p.dim() == 1:
                p.copy_((torch.randn(p.shape, generator=g) * 0.1 + (1.0 if centred(name) else 0.0)).to(p.device))
    return mod


# ---- fixtures, bound at module level by the files that use them --------------------------------------------------------------
def restore_mode(also=None):
    """an autouse fixture that puts the default compute mode back after each test; also = (object, attribute): that attribute
    gets the value it had before the test"""
    @pytest.fixture(autouse=True)
    def _restore_mode():
        import rosettafold_pytorch_amd as R
        saved = getattr(*also) if also else None
        yield
        if also:
            setattr(*also, saved)
        R.set_compute_dtype(torch.bfloat16)
    return _restore_mode


@pytest.fixture(params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def h16(request):
    """both 16-bit builds of the library"""
    import rosettafold_pytorch_amd as R
    R.set_compute_dtype(request.param)
    yield request.param
    R.set_compute_dtype(torch.bfloat16)


def records_fixture(env_name, records, yardstick):
    """an autouse module fixture: with the environment variable set to a file, what `held` appended to `records` is merged into
    that JSON document under "kernel_errors" when the module is done"""
    @pytest.fixture(scope="module", autouse=True)
    def _write_records():
        yield
        path = os.environ.get(env_name)
        if path and records:
            doc = {}
            if os.path.exists(path):
                with open(path) as fh:
                    doc = json.load(fh)
            doc["kernel_errors"] = {"margin": MARGIN, "yardstick": yardstick, "cases": records}
            with open(path, "w") as fh:
                json.dump(doc, fh, indent=1)
    return _write_records


# ---- the yardstick rule ----------------------------------------------------------------------------------------------------------
def errors(got, want, rows=1):
    """(relative L2 error of the whole tensor, worst relative L2 error of one row); inf where `want` is exactly zero and `got`
    is not"""
    g, w = got.detach().double().cpu(), want.detach().double().cpu()
    assert g.shape == w.shape and torch.isfinite(g).all()
    if rows == "bl":
        if g.dim() == 4:
            g, w = g.permute(0, 2, 1, 3), w.permute(0, 2, 1, 3)
        rows = g.dim() - 2
    lead = g.shape[:g.dim() - rows]
    gr, wr = g.reshape(*lead, -1), w.reshape(*lead, -1)
    num, den = (gr - wr).norm(dim=-1), wr.norm(dim=-1)
    worst = torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, float("inf"), 0.0).double()).max().item()
    if w.norm() > 0:
        return ((g - w).norm() / w.norm()).item(), worst
    return (float("inf") if (g != 0).any() else 0.0), worst


def held(got, ref64, ref32, tag, units, rows, records, key="grad"):
    """every output named in ref64 under MARGIN x its yardstick, whole tensor and worst row.  units and rows: one value for all
    outputs or a dict per output.  Prints the figures and appends them to `records` under the key name the file's JSON uses."""
    ok = True
    for n in ref64:
        unit = units[n] if isinstance(units, dict) else units
        cut = rows[n] if isinstance(rows, dict) else rows
        m_all, m_row = errors(got[n], ref64[n], cut)
        y_all, y_row = errors(ref32[n], ref64[n], cut)
        c_all, c_row = MARGIN * max(y_all, unit), MARGIN * max(y_row, unit)
        print(f"{tag} {n}: rel-L2 {m_all:.3e} (float32 autograd {y_all:.3e}, unit {unit:.1e}, ceiling {c_all:.3e}), "
              f"worst row {m_row:.3e} (float32 autograd {y_row:.3e}, ceiling {c_row:.3e})")
        records.append({"case": tag, key: n, "rel_l2": m_all, "worst_row": m_row, "f32_autograd_rel_l2": y_all,
                        "f32_autograd_worst_row": y_row, "unit": unit, "ceiling_rel_l2": c_all, "ceiling_worst_row": c_row})
        ok = ok and m_all <= c_all and m_row <= c_row
    return ok


# ---- the ceiling-or-kink-floor rule ------------------------------------------------------------------------------------------------
def oracle_grads(fn, P, inputs, loss, unit=None, seed=0, fixed=(), frozen=(), missing="absent"):
    """float64 autograd on the CPU of loss(fn(P, *inputs.values())): ({parameter name or input name: gradient}, kink floors).
    loss: a weight tensor w for sum(out * w), or a callable on what fn returns.  missing: a parameter or input the loss does not
    reach is "absent" from the result or holds "zeros".  With unit (UNIT[mode]) the second value is each gradient's relative
    change under the jitter of the module's docstring; without it, None."""
    assert missing in ("absent", "zeros")

    def run(P, xs):
        P = {k: v.detach().clone().requires_grad_(k not in frozen) for k, v in P.items()}
        xs = {k: v.detach().double().cpu().clone().requires_grad_() for k, v in xs.items()}
        out = fn(P, *xs.values())
        (loss(out) if callable(loss) else (out * loss.double().cpu()).sum()).backward()
        leaves = {**{k: v for k, v in P.items() if k not in frozen}, **xs}
        if missing == "zeros":
            return {k: v.grad if v.grad is not None else torch.zeros_like(v) for k, v in leaves.items()}
        return {k: v.grad for k, v in leaves.items() if v.grad is not None}

    ref = run(P, inputs)
    if unit is None:
        return ref, None
    g = gen(seed + 1000)
    jit = lambda t: t.double().cpu() * (1 + unit * (2 * torch.rand(t.shape, generator=g, dtype=torch.float64) - 1))  # noqa: E731
    Pj = {k: jit(v) for k, v in P.items()}
    refj = run(Pj, {k: v if k in fixed else jit(v.detach()) for k, v in inputs.items()})
    return ref, {k: rel(refj[k], ref[k]) for k in ref}


def tolerance(dtype, floor, key):
    return max(CEIL[dtype], 3 * floor[key]) if floor is not None else CEIL[dtype]


def compare(got, ref, dtype, tag, floor=None, zero=None, norms=None, unreached_zero=False):
    """every gradient of `ref` against got[key]: relative L2 error < tolerance(dtype, floor, key).  Prints one line per gradient,
    collects the failures and asserts once.  zero = {key: noise bound}: got[key] is exactly zero and the oracle's own norm lies
    below the bound.  norms = {key: size}: the error of got[key] is taken against `size` under CEIL, and the oracle's own norm
    lies below 1e-10 x size.  unreached_zero: whatever `got` holds and `ref` does not is exactly zero."""
    zero, norms = zero or {}, norms or {}
    assert set(ref) <= set(got), set(ref) - set(got)
    if unreached_zero:
        for key in set(got) - set(ref):
            assert (got[key] == 0).all(), key
    bad = {}
    for key in ref:
        if key in zero:
            assert (got[key] == 0).all(), key
            assert ref[key].norm() < zero[key], (key, ref[key].norm(), zero[key])
            continue
        if key in norms:
            assert ref[key].norm().item() < 1e-10 * norms[key], (key, ref[key].norm().item(), norms[key])
            err, tol = (got[key].detach().double().cpu() - ref[key]).norm().item() / norms[key], CEIL[dtype]
        else:
            err, tol = rel(got[key], ref[key]), tolerance(dtype, floor, key)
        kink = f", kink floor {floor[key]:.3e}" if floor is not None and key not in norms else ""
        print(f"{dtype} {tag} {key}: rel-L2 {err:.3e} (tolerance {tol:.3e}{kink})")
        if not err < tol:
            bad[key] = (err, tol)
    assert not bad, (tag, bad)


# ---- the device side ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def recording(mod, train=False):
    """mod on the device with its backward switched on (and in train() mode); switched off, in eval() mode and back on the CPU
    afterwards, whatever happened"""
    mod.to(DEV)
    try:
        yield (mod.train() if train else mod).enable_backward()
    finally:
        (mod.eval() if train else mod).enable_backward(False)
        mod.to("cpu")


def grads_of(mod, inputs, loss, scale=1.0, leaves=None, pre="m"):
    """clear every .grad, run mod(*inputs.values()) on the device and (loss * scale).backward(): ({pre.name: parameter gradient,
    input name: leaf gradient}, the detached output).  inputs: name -> tensor or None in call order; leaves: the names that
    require grad (default: every floating-point input).  loss: a weight tensor w for sum(out * w), or a callable on the output."""
    for p in mod.parameters():
        p.grad = None
    if leaves is None:
        leaves = [k for k, v in inputs.items() if v is not None and v.is_floating_point()]
    xs = {k: v if v is None else v.detach().to(DEV).requires_grad_(k in leaves) for k, v in inputs.items()}
    out = mod(*xs.values())
    ((loss(out) if callable(loss) else (out * loss.to(DEV)).sum()) * scale).backward()
    grads = {f"{pre}.{n}": p.grad for n, p in mod.named_parameters()}
    grads.update({k: xs[k].grad for k in leaves})
    detach = lambda o: o.detach() if torch.is_tensor(o) else o  # noqa: E731
    out = {k: detach(o) for k, o in out.items()} if isinstance(out, dict) else (
        tuple(detach(o) for o in out) if isinstance(out, tuple) else detach(out))
    return grads, out
