"""Backward pass of MsaEmbedding and PairEmbedding (enable_backward): every parameter gradient, and the template's, against
float64 autograd through the CPU oracle (oracle/rf_oracle.py: msa_embedding, pair_embedding) in the three compute modes, with
loss = sum(module(...) * w) for a random w; unchanged forward numbers, exact zeros for residue types absent from the input,
dropout replay in train() mode, fp16 small losses, determinism and the refusals.

Ceilings (relative L2 error of a whole gradient): everything outside the template branch is exact fp32 arithmetic on the output
gradient in every mode and is held to 1e-4 in every mode -- the first 2h + 1 columns of proj.weight.grad as a block of their own;
the template columns of proj.weight.grad, ln_template.* and template.grad follow the compute mode and are held to the project's
ceilings, 1e-4 (fp32) / 1e-2 (fp16) / 5e-2 (bf16).  These per-block ceilings, held with `<=`, are this file's own; the references
and the device side come from tests/grad_oracle.py."""
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
MODES, CEIL = G.MODES, G.CEIL
EXACT = 1e-4
MAX_LEN = 260
V = 21
ABSENT = 5   # a residue type no test input contains
# MsaEmbedding (B, N, L, d_msa): two samples with an odd chain; one MSA row (query_enc's second row gets exactly nothing) with a
# width that is no multiple of 32; the model's width (six channel tiles of the kernel).
MSA_SHAPES = [(2, 3, 13, 32), (1, 1, 7, 24), (1, 4, 64, 384)]
# PairEmbedding (B, L, d_pair, d_template; 0: no template).  L = 1; d_pair = 20 is no multiple of 8 and works without a
# template; a template narrower than a wave on an odd chain; the model's widths.
PAIR_SHAPES = [(2, 13, 32, 0), (1, 1, 16, 0), (1, 13, 20, 0), (1, 37, 72, 16), (1, 24, 288, 64)]
TEMPLATE_KEYS = ("m.ln_template.weight", "m.ln_template.bias", "template", "m.proj.weight[template]")


_restore_mode = G.restore_mode()


def tokens(shape, g):
    t = torch.randint(0, V, shape, generator=g)
    t[t == ABSENT] = ABSENT + 1
    return t


def residue_numbers(B, L, g):
    """strictly increasing with gaps of 1..3 (below MAX_LEN at every test length)"""
    return torch.randint(1, 4, (B, L), generator=g).cumsum(-1)


# ================================================================================================ MsaEmbedding
@functools.lru_cache(maxsize=None)
def msa_setup(shape, p_drop=0.1):
    """module (fp32 weights, CPU) and inputs, shared by the modes and left unchanged"""
    B, N, L, D = shape
    torch.manual_seed(100 + 17 * L + D)
    mod = R.MsaEmbedding(d_input=V, d_msa=D, max_len=MAX_LEN, p_pe_drop=p_drop)
    g = G.gen(300 + 17 * L + D)
    return mod, tokens((B, N, L), g), residue_numbers(B, L, g), torch.randn(B, N, L, D, generator=g)


@functools.lru_cache(maxsize=None)
def msa_reference(shape):
    mod, msa, aa_idx, w = msa_setup(shape)
    return G.oracle_grads(lambda P: O.msa_embedding(P, "m", msa, aa_idx, MAX_LEN), G.state(mod), {}, w)[0]


def msa_backward(mod, msa, aa_idx, w, scale=1.0):
    return G.grads_of(mod, {"msa": msa, "aa_idx": aa_idx}, w, scale)[0]


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("shape", MSA_SHAPES, ids=str)
def test_msa_embedding_grads_against_oracle(dtype, shape):
    R.set_compute_dtype(dtype)
    mod, msa, aa_idx, w = msa_setup(shape)
    ref = msa_reference(shape)
    with G.recording(mod):
        got = msa_backward(mod, msa, aa_idx, w)
    assert set(got) == set(ref) == {"m.to_embedding.weight", "m.query_enc.weight"}
    for key in ref:
        err = G.rel(got[key], ref[key])
        print(f"{dtype} MsaEmbedding {shape} {key}: rel-L2 {err:.3e} (ceiling {EXACT:.0e})")
        assert err <= EXACT, (key, err)
    used = torch.zeros(V, dtype=torch.bool)
    used[msa.view(-1)] = True
    assert not used[ABSENT]
    table = got["m.to_embedding.weight"].cpu()
    assert (table[~used] == 0).all() and (table[used] != 0).any(-1).all()   # residue types absent from the input: exact zeros
    if shape[1] == 1:
        assert (got["m.query_enc.weight"][1] == 0).all()


# ================================================================================================ PairEmbedding
@functools.lru_cache(maxsize=None)
def pair_setup(shape):
    B, L, D, Dt = shape
    torch.manual_seed(500 + 17 * L + D)
    mod = G.randomize(R.PairEmbedding(d_input=V, d_pair=D, max_len=MAX_LEN, use_template=Dt > 0, d_template=Dt or 64), 600 + L + D,
                      lambda name: name.endswith("weight"))
    g = G.gen(700 + 17 * L + D)
    seq, aa_idx = tokens((B, L), g), residue_numbers(B, L, g)
    template = torch.randn(B, L, L, Dt, generator=g) * 2 + 0.5 if Dt else None
    return mod, seq, aa_idx, template, torch.randn(B, L, L, D, generator=g)


def split_proj(grads, h):
    """proj.weight's gradient as its two blocks: the sequence and separation columns, and the template columns (when there are any)"""
    out = dict(grads)
    full = out.pop("m.proj.weight")
    out["m.proj.weight[seq|sep]"] = full[:, :2 * h + 1]
    if full.shape[1] > 2 * h + 1:
        out["m.proj.weight[template]"] = full[:, 2 * h + 1:]
    return out


@functools.lru_cache(maxsize=None)
def pair_reference(shape):
    mod, seq, aa_idx, template, w = pair_setup(shape)
    fn = lambda P, t64=None: O.pair_embedding(P, "m", seq, aa_idx, MAX_LEN, template=t64)  # noqa: E731
    out, _ = G.oracle_grads(fn, G.state(mod), {} if template is None else {"template": template}, w)
    return split_proj(out, mod.half_d_pair)


def pair_backward(mod, seq, aa_idx, template, w, scale=1.0):
    out, _ = G.grads_of(mod, {"seq": seq, "aa_idx": aa_idx, "template": template}, w, scale)
    return split_proj(out, mod.half_d_pair)


def check_pair(got, ref, dtype, shape, factor=1.0):
    assert set(got) == set(ref)
    bad = {}
    for key in ref:
        ceil = CEIL[dtype] if key in TEMPLATE_KEYS else EXACT
        err = G.rel(got[key] * factor, ref[key])
        print(f"{dtype} PairEmbedding {shape} {key}: rel-L2 {err:.3e} (ceiling {ceil:.0e})")
        if not err <= ceil:
            bad[key] = (err, ceil)
    assert not bad, bad


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("shape", PAIR_SHAPES, ids=str)
def test_pair_embedding_grads_against_oracle(dtype, shape):
    R.set_compute_dtype(dtype)
    mod, seq, aa_idx, template, w = pair_setup(shape)
    ref = pair_reference(shape)
    with G.recording(mod):
        got = pair_backward(mod, seq, aa_idx, template, w)
    check_pair(got, ref, dtype, shape)
    assert ("template" in got) == (shape[3] > 0)
    used = torch.zeros(V, dtype=torch.bool)
    used[seq.view(-1)] = True
    assert not used[ABSENT]
    assert (got["m.embed_seq.weight"].cpu()[~used] == 0).all()   # residue types absent from the input: exact zeros
    if shape[1] == 1:                                             # L = 1: log(1) = 0, the separation column gets exactly nothing
        assert (got["m.proj.weight[seq|sep]"][:, -1] == 0).all()


# ================================================================================================ forward unchanged
@pytest.mark.parametrize("dtype", MODES)
def test_recording_forward_is_bitwise_unchanged(dtype):
    R.set_compute_dtype(dtype)
    for setup, shape in ((msa_setup, MSA_SHAPES[0]), (pair_setup, PAIR_SHAPES[0]), (pair_setup, PAIR_SHAPES[3])):
        mod, *inputs, _ = setup(shape)
        mod = mod.to(DEV)
        try:
            a = [t.to(DEV) if t is not None else None for t in inputs]
            with torch.no_grad():
                ref = mod(*a)
            plain = mod(*a)                # grad mode on, not opted in: nothing records
            assert not plain.requires_grad and torch.equal(plain, ref)
            mod.enable_backward()
            out = mod(*a)
            assert out.requires_grad and torch.equal(out.detach(), ref)
            with torch.no_grad():          # opted in, no grad mode: nothing records either
                assert torch.equal(mod(*a), ref)
            assert torch.equal(mod.run(*a), ref)   # what the trunk calls: run() without a tape
        finally:
            mod.enable_backward(False)
            mod.to("cpu")


# ================================================================================================ training mode
def test_msa_embedding_replays_its_dropout():
    """train(): d to_embedding is the index_add of keep / (1 - p) * w, with keep read off the recorded forward's own output
    (a dropped element is the query encoding alone) and checked against the eval-mode output; d query_enc does not see the mask."""
    R.set_compute_dtype(torch.float32)
    shape, p = MSA_SHAPES[0], 0.3
    B, N, L, D = shape
    mod, msa, aa_idx, w = msa_setup(shape, p)
    mod = mod.to(DEV)
    try:
        mod.enable_backward()
        eval_grads = msa_backward(mod, msa, aa_idx, w)
        with torch.no_grad():
            y_eval = mod(msa.to(DEV), aa_idx.to(DEV))
        mod.train()
        for p_ in mod.parameters():
            p_.grad = None
        R.manual_seed(11)
        y = mod(msa.to(DEV), aa_idx.to(DEV))
        (y * w.to(DEV)).sum().backward()
        q = mod.query_enc.weight.detach()[(torch.arange(N) > 0).long().to(DEV)][None, :, None, :]
        keep = (y.detach() != q).expand(B, N, L, D)
        frac = keep.float().mean().item()
        assert abs(frac - (1 - p)) < 0.05, frac                                     # the dropout acts, at its rate
        kept_ok = torch.where(keep, (y.detach() - q) * (1 - p) - (y_eval - q), torch.zeros_like(y_eval))
        assert kept_ok.abs().max().item() <= 1e-5 * (y_eval - q).abs().max().item()   # a kept element is the eval value / (1 - p)
        want = torch.zeros(V, D, dtype=torch.float64).index_add_(
            0, msa.view(-1), (keep.cpu().double() / (1 - p) * w.double()).view(-1, D))
        err = G.rel(mod.to_embedding.weight.grad, want)
        print(f"train-mode d to_embedding: rel-L2 {err:.3e}")
        assert err <= EXACT
        assert torch.equal(mod.query_enc.weight.grad, eval_grads["m.query_enc.weight"])
        assert not torch.equal(mod.to_embedding.weight.grad, eval_grads["m.to_embedding.weight"])
        first = mod.to_embedding.weight.grad.clone()     # the same seed: the same mask, the same bits
        for p_ in mod.parameters():
            p_.grad = None
        R.manual_seed(11)
        (mod(msa.to(DEV), aa_idx.to(DEV)) * w.to(DEV)).sum().backward()
        assert torch.equal(mod.to_embedding.weight.grad, first)
    finally:
        mod.eval().enable_backward(False)
        mod.to("cpu")


# ================================================================================================ fp16 small losses
def test_fp16_small_loss_does_not_underflow():
    """a loss scaled by 2^-20: the gradients times 2^20 stay within the same ceilings"""
    R.set_compute_dtype(torch.float16)
    scale = 2.0 ** -20
    shape = PAIR_SHAPES[3]
    mod, seq, aa_idx, template, w = pair_setup(shape)
    with G.recording(mod):
        got = pair_backward(mod, seq, aa_idx, template, w, scale=scale)
    assert all(torch.isfinite(g_).all() and g_.abs().max() > 0 for g_ in got.values())
    check_pair(got, pair_reference(shape), torch.float16, shape, factor=1 / scale)
    mshape = MSA_SHAPES[0]
    mod, msa, aa_idx, w = msa_setup(mshape)
    with G.recording(mod):
        got = msa_backward(mod, msa, aa_idx, w, scale=scale)
    for key, want in msa_reference(mshape).items():
        assert G.rel(got[key] / scale, want) <= EXACT, key


# ================================================================================================ determinism
def test_backward_is_deterministic():
    R.set_compute_dtype(torch.bfloat16)
    for setup, run, shape in ((msa_setup, msa_backward, MSA_SHAPES[2]), (pair_setup, pair_backward, PAIR_SHAPES[3])):
        mod, *inputs = setup(shape)
        with G.recording(mod):
            res = [{k: v.clone() for k, v in run(mod, *inputs).items()} for _ in range(2)]
        assert res[0].keys() == res[1].keys() and all(torch.equal(res[0][k], res[1][k]) for k in res[0])


# ================================================================================================ refusals
def test_template_widths_refused_while_recording_only():
    """d_template = 12 is fine for the fp32 forward, refused while recording (the template branch's 16-bit operands); d_pair = 20
    without a template records (PAIR_SHAPES[2])"""
    R.set_compute_dtype(torch.float32)
    torch.manual_seed(9)
    g = G.gen(9)
    mod = R.PairEmbedding(d_input=V, d_pair=32, max_len=MAX_LEN, use_template=True, d_template=12).to(DEV)
    seq, aa_idx = tokens((1, 6), g).to(DEV), residue_numbers(1, 6, g).to(DEV)
    template = torch.randn(1, 6, 6, 12, generator=g).to(DEV)
    with torch.no_grad():
        plain = mod(seq, aa_idx, template)
    mod.enable_backward()
    with pytest.raises(ValueError):
        mod(seq, aa_idx, template)
    with pytest.raises(ValueError):
        mod.run(seq, aa_idx, template, tape={})
    with torch.no_grad():              # without grad mode the same module runs
        assert torch.equal(mod(seq, aa_idx, template), plain)
    assert torch.equal(mod.run(seq, aa_idx, template), plain)


def test_index_validation_is_kept_while_opted_in():
    R.set_compute_dtype(torch.float32)
    g = G.gen(10)
    msa_mod = R.MsaEmbedding(d_input=V, d_msa=32, max_len=MAX_LEN).to(DEV).enable_backward()
    pair_mod = R.PairEmbedding(d_input=V, d_pair=32, max_len=MAX_LEN).to(DEV).enable_backward()
    msa, aa_idx = tokens((1, 2, 6), g).to(DEV), residue_numbers(1, 6, g).to(DEV)
    bad_msa = msa.clone()
    bad_msa[0, 0, 3] = V
    bad_idx = aa_idx.clone()
    bad_idx[0, -1] = MAX_LEN
    for args in ((bad_msa, aa_idx), (msa, bad_idx)):
        with pytest.raises(IndexError):
            msa_mod(*args)
    for args in ((bad_msa[:, 0], aa_idx), (msa[:, 0], bad_idx)):
        with pytest.raises(IndexError):
            pair_mod(*args)
    with pytest.raises(ValueError):    # the template rules of forward() too
        pair_mod(msa[:, 0], aa_idx, torch.zeros(1, 6, 6, 64, device=DEV))
    assert msa_mod(msa, aa_idx).requires_grad and pair_mod(msa[:, 0], aa_idx).requires_grad
