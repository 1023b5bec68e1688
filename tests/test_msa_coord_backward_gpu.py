"""Backward pass of MsaUpdateWithPairAndCoord (enable_backward): the module's gradients against float64 autograd through the CPU
oracle (oracle/rf_oracle.py: msa_update_with_pair_and_coord) in the three compute modes, unchanged forward numbers, the exact
facts (to_k.bias, xyz, L = 1), dropout replay (finite differences), fp16 small losses, determinism and the refusal.

Tolerance: the ceiling-or-kink-floor rule of tests/grad_oracle.py; the feed-forward's ReLU is the kink, and the jitter falls on
state, msa and every parameter.  xyz is never jittered: it enters through the distance mask alone, and every case asserts on the
CPU that each pairwise CA distance is at least 1e-4 A away from every bin, so that the float64 mask is the kernels' (the fp32
distance error at these ranges is about 1e-5).  to_k.bias adds q_i . b_k to every logit of a row and drops out of the softmax:
an exact zero here, rounding noise in the oracle."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import grad_oracle as G  # noqa: E402
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import ops  # noqa: E402
from oracle import rf_oracle as O  # noqa: E402

DEV = "cuda"
MODES, CEIL, UNIT = G.MODES, G.CEIL, G.UNIT
BINS = (8.0, 12.0, 16.0, 20.0)
GAP = 1e-4
# (B, N, L, d_msa, d_state) -> seed of the coordinates (chosen so that the preconditions below hold).  L = 65: no multiple of 8
# nor of a wave, two samples (in the 16-bit modes the map and v^T stay fp32 there: the 16-bit GEMM contracts over multiples of
# 8); WIDE: the model's width.
SHAPES = {(1, 3, 24, 32, 16): 2, (2, 2, 65, 64, 32): 0}
WIDE, WIDE_SEED = (1, 4, 64, 384, 32), 0


CENTRED = lambda name: name.endswith("weight")   # noqa: E731  the 1-D parameters drawn around 1
_restore_mode = G.restore_mode()


def coordinates(B, L, seed):
    """fp32 [B, L, 3, 3]: CA (atom 1) a random walk of 3.8 A steps, N and C at unit noise around it; asserts the preconditions"""
    g_ = G.gen(7300 + seed)
    step = torch.randn(B, L, 3, generator=g_)
    ca = (3.8 * step / step.norm(dim=-1, keepdim=True)).cumsum(1)
    xyz = (ca[:, :, None, :] + torch.randn(B, L, 3, 3, generator=g_) * torch.tensor([1.0, 0.0, 1.0])[:, None]).float().contiguous()
    cad = xyz[:, :, 1].double()
    dist = (cad[:, :, None] - cad[:, None]).norm(dim=-1)
    b_ = torch.tensor(BINS, dtype=torch.float64)
    gap = (dist[:, None] - b_[None, :, None, None]).abs().min().item()
    assert gap >= GAP, f"a CA distance lies {gap:.2e} A from a bin: choose another seed"
    if L >= 24:
        mask = dist[:, None] < b_[None, :, None, None]
        off = ~torch.eye(L, dtype=torch.bool)
        per_head = lambda m: (m & off).transpose(0, 1).flatten(1).any(-1).all()   # noqa: E731
        assert per_head(mask) and per_head(~mask), "a head is all in or all out of range"
    return xyz


@functools.lru_cache(maxsize=None)
def setup(shape, seed, p_dropout=0.0):
    """module (fp32 weights, CPU) and inputs, shared by the modes and left unchanged"""
    B, N, L, D, Ds = shape
    torch.manual_seed(100 + seed)
    mod = G.randomize(R.MsaUpdateWithPairAndCoord(D, Ds, 32, 4 * D, p_dropout=p_dropout), 200 + seed, CENTRED)
    g = G.gen(300 + seed)
    xyz = coordinates(B, L, seed)
    st, msa = torch.randn(B, L, Ds, generator=g), torch.randn(B, N, L, D, generator=g)
    return mod, xyz, st, msa, torch.randn(B, N, L, D, generator=g)


@functools.lru_cache(maxsize=None)
def reference(shape, seed, dtype):
    """float64 autograd through the oracle and the kink floors; xyz takes part as an input that is never jittered"""
    mod, xyz, st, msa, w = setup(shape, seed)
    fn = lambda P, xd, sd, md: O.msa_update_with_pair_and_coord(P, "m", xd, sd, md)  # noqa: E731
    return G.oracle_grads(fn, G.state(mod), {"xyz": xyz, "state": st, "msa": msa}, w, UNIT[dtype], seed, fixed=("xyz",))


def backward_of(mod, xyz, st, msa, w, scale=1.0, xyz_grad=False):
    """loss.backward() on the device: {"state", "msa", "m." + name: gradient} (and "xyz" with xyz_grad)"""
    leaves = ("xyz", "state", "msa") if xyz_grad else ("state", "msa")
    return G.grads_of(mod, {"xyz": xyz, "state": st, "msa": msa}, w, scale, leaves)[0]


def check_against_oracle(shape, seed, dtype):
    R.set_compute_dtype(dtype)
    mod, xyz, st, msa, w = setup(shape, seed)
    ref, floor = reference(shape, seed, dtype)
    assert "xyz" not in ref   # the oracle's autograd gives xyz no gradient: the mask is piecewise constant
    with G.recording(mod):
        got = backward_of(mod, xyz, st, msa, w, xyz_grad=True)
    assert got.pop("xyz") is None
    assert {k for k, g_ in got.items() if g_ is not None} == set(ref)
    G.compare(got, ref, dtype, str(shape), floor, zero={"m.to_k.bias": 1e-9 * ref["m.to_q.bias"].norm()})


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("shape", list(SHAPES), ids=str)
def test_grads_against_oracle(dtype, shape):
    check_against_oracle(shape, SHAPES[shape], dtype)


def test_grads_against_oracle_at_the_models_width():
    """d_msa 384, d_state 32 in the default mode.  (These 256 rows take the two-GEMM feed-forward: the fused kernel starts at
    16384 rows, where a float64 oracle takes minutes -- the test below covers what it records.)"""
    check_against_oracle(WIDE, WIDE_SEED, torch.bfloat16)


def test_fused_feed_forward_records_the_same_gradients(monkeypatch):
    """16384 rows of width 384 in the default mode: the fused feed-forward is what records.  The backward rebuilds the hidden
    activations from the saved input whichever forward ran, so every gradient has the bits of the two-GEMM route's -- which the
    tests above hold against the oracle."""
    R.set_compute_dtype(torch.bfloat16)
    shape = (1, 64, 256, 384, 32)
    B, N, L, D, _ = shape
    x = torch.zeros(B, N, L, D, device=DEV)
    mod, xyz, st, msa, w = setup(shape, WIDE_SEED)
    with G.recording(mod):
        assert ops.ffn_fused_applies(x.to(torch.bfloat16), x, D, 4 * D)
        fused = [g_.clone() for g_ in backward_of(mod, xyz, st, msa, w).values()]
        monkeypatch.setattr(ops, "FUSE_FFN", False)
        assert not ops.ffn_fused_applies(x.to(torch.bfloat16), x, D, 4 * D)
        plain = [g_.clone() for g_ in backward_of(mod, xyz, st, msa, w).values()]   # (before the module, and its .grad, move)
    assert all(torch.isfinite(a).all() for a in fused) and (fused[-2] != 0).any()   # (d state)
    assert all(torch.equal(a, b) for a, b in zip(fused, plain))


# ------------------------------------------------------------------------------------------------ exact facts
def test_one_residue_gives_state_an_exact_zero():
    """L = 1: the softmax is the constant 1 whatever q and k are, so state receives exactly nothing (and msa still does)"""
    R.set_compute_dtype(torch.float32)
    torch.manual_seed(5)
    mod = G.randomize(R.MsaUpdateWithPairAndCoord(32, 16, 32, 128, p_dropout=0.0), 5, CENTRED).to(DEV).enable_backward()
    g = G.gen(5)
    xyz, st, msa = torch.randn(2, 1, 3, 3, generator=g), torch.randn(2, 1, 16, generator=g), torch.randn(2, 3, 1, 32, generator=g)
    grads = backward_of(mod, xyz, st, msa, torch.randn(2, 3, 1, 32, generator=g))
    assert grads["state"] is not None and (grads["state"] == 0).all()
    assert (grads["msa"] != 0).any()
    for n in ("to_q.weight", "to_q.bias", "to_k.weight", "to_k.bias", "ln_state.weight", "ln_state.bias"):
        assert (grads["m." + n] == 0).all(), n


# ------------------------------------------------------------------------------------------------ forward unchanged
@pytest.mark.parametrize("dtype", MODES)
def test_recording_forward_is_bitwise_unchanged(dtype):
    R.set_compute_dtype(dtype)
    shape = (2, 2, 65, 64, 32)
    mod, xyz, st, msa, _ = setup(shape, SHAPES[shape])
    mod = mod.to(DEV)
    try:
        a = tuple(t.to(DEV) for t in (xyz, st, msa))
        with torch.no_grad():
            ref = mod(*a)
        plain = mod(*a)            # grad mode on, not opted in: nothing records
        assert not plain.requires_grad and torch.equal(plain, ref)
        mod.enable_backward()
        out = mod(a[0], a[1].clone().requires_grad_(), a[2].clone().requires_grad_())
        assert out.requires_grad and torch.equal(out.detach(), ref)
        with torch.no_grad():      # opted in, no grad mode: nothing records either
            assert torch.equal(mod(*a), ref)
        assert torch.equal(mod.run(*a), ref)   # what the trunk calls: no tape
    finally:
        mod.enable_backward(False)
        mod.to("cpu")


# ------------------------------------------------------------------------------------------------ training mode
def test_dropout_replay_finite_differences():
    """train(), fp32: the feed-forward's dropout is replayed -- a central finite difference along a random direction agrees with
    the analytic value (form and bound of tests/test_axial_backward_gpu.py::test_dropout_replay_finite_differences)"""
    R.set_compute_dtype(torch.float32)
    shape, seed = (1, 3, 24, 32, 16), SHAPES[(1, 3, 24, 32, 16)]
    mod, xyz, st, msa, w = setup(shape, seed, 0.2)
    with G.recording(mod, train=True):
        xyz, st, msa, w = (t.to(DEV) for t in (xyz, st, msa, w))
        g = G.gen(31)
        vs, vm = torch.randn(st.shape, generator=g).to(DEV), torch.randn(msa.shape, generator=g).to(DEV)

        def loss(s_, m_):
            R.manual_seed(5)
            return (mod(xyz, s_, m_) * w).sum()

        with torch.no_grad():
            mod.eval()
            plain = (mod(xyz, st, msa) * w).sum()
            mod.train()
            assert not torch.equal(loss(st, msa), plain)   # the dropout acts
        for p in mod.parameters():
            p.grad = None
        sg, mg = st.clone().requires_grad_(), msa.clone().requires_grad_()
        loss(sg, mg).backward()
        eps = 1e-3   # (small against the ReLU kinks a central difference steps across; fp32 loss noise ~1e-5)
        with torch.no_grad():
            fd = (loss(st + eps * vs, msa + eps * vm) - loss(st - eps * vs, msa - eps * vm)).item() / (2 * eps)
        an = ((sg.grad * vs).sum() + (mg.grad * vm).sum()).item()
        assert abs(fd - an) <= 2e-2 * abs(an) + 1e-3, (fd, an)
        wq = mod.to_q.weight
        dw = torch.randn(wq.shape, generator=g).to(DEV) * 0.1
        with torch.no_grad():
            w0 = wq.clone()
            wq.copy_(w0 + eps * dw)
            lp = loss(st, msa).item()
            wq.copy_(w0 - eps * dw)
            lm = loss(st, msa).item()
            wq.copy_(w0)
        an_w = (mod.to_q.weight.grad * dw).sum().item()
        assert abs((lp - lm) / (2 * eps) - an_w) <= 2e-2 * abs(an_w) + 1e-3, ((lp - lm) / (2 * eps), an_w)


# ------------------------------------------------------------------------------------------------ fp16 small losses
def test_fp16_small_loss_does_not_underflow():
    R.set_compute_dtype(torch.float16)
    shape = (1, 3, 24, 32, 16)
    mod, xyz, st, msa, w = setup(shape, SHAPES[shape])
    with G.recording(mod):
        res = [backward_of(mod, xyz, st, msa, w, scale=scale) for scale in (1.0, 1e-6)]
    for key, a in res[0].items():
        b = res[1][key]
        assert torch.isfinite(b).all(), key
        if key == "m.to_k.bias":
            assert (b == 0).all()
            continue
        assert b.abs().max() > 0, key
        assert G.rel(b * 1e6, a) < CEIL[torch.float16], key


# ------------------------------------------------------------------------------------------------ determinism
def test_backward_is_deterministic():
    R.set_compute_dtype(torch.bfloat16)
    shape = (2, 2, 65, 64, 32)
    mod, xyz, st, msa, w = setup(shape, SHAPES[shape])
    with G.recording(mod):
        res = [[g_.clone() for g_ in backward_of(mod, xyz, st, msa, w).values()] for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*res))


# ------------------------------------------------------------------------------------------------ refusals
def test_channel_counts_checked_while_recording():
    R.set_compute_dtype(torch.float32)
    torch.manual_seed(7)
    mod = R.MsaUpdateWithPairAndCoord(36, 16, 32, 144, p_dropout=0.0).to(DEV)
    g = G.gen(7)
    xyz, st, msa = (torch.randn(s, generator=g).to(DEV) for s in ((1, 8, 3, 3), (1, 8, 16), (1, 2, 8, 36)))
    with torch.no_grad():
        plain = mod(xyz, st, msa)   # d_msa = 36 is fine for the forward
    mod.enable_backward()
    with pytest.raises(ValueError):
        mod(xyz, st.requires_grad_(), msa)
    with pytest.raises(ValueError):
        mod.run(xyz, st.detach(), msa, tape={})
    with torch.no_grad():
        assert torch.equal(mod(xyz, st, msa), plain)
