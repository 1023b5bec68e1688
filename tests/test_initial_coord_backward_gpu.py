"""Backward pass of PositionWiseWeightFactor and InitialCoordGenerationWithMsaAndPair (enable_backward; rf.py:184-217, 679-749)
through the public surface, against the oracle's float64 autograd (O.poswise_weight, O.initial_coord_generation).

Every parameter gradient and both input gradients are held by the ceiling-or-kink-floor rule of tests/grad_oracle.py (a parameter
the loss does not reach counts as a zero gradient).  to_k's bias moves every logit of a softmax by the same amount, so its exact
gradient is zero and a relative error has no denominator: in the coordinate module (where the bias never reaches a kernel) the
gradient must be exactly zero; in PositionWiseWeightFactor it is sum_{b,n,l} dk, and its norm must stay under the mode's ceiling
times the norm of sum_{b,n,l} |dk| -- the size of the terms that cancel (dk = the float64 gradient of to_k's output); the float64
reference's own value is checked against the same bound first.  The blocks' node_to_k.bias is taken against node_to_k.weight's
gradient norm per input channel, as in tests/test_graph_backward_gpu.py."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import grad_oracle as G  # noqa: E402
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import ops  # noqa: E402
from rosettafold_pytorch_amd.runtime import RT  # noqa: E402
from oracle import rf_oracle as O  # noqa: E402

DEV = "cuda"
MODES, MODE_IDS, CEIL, UNIT = G.MODES, G.MODE_IDS, G.CEIL, G.UNIT
# PositionWiseWeightFactor: (d_msa, H, N, L)
PW_CASES = [(24, 3, 3, 7), (96, 12, 5, 16)]
# InitialCoordGenerationWithMsaAndPair: (d_msa, d_pair, d_node, d_edge, heads, layers, B, N, L); the first is the golden's size
IC_CASES = [(16, 16, 8, 8, 4, 2, 2, 3, 7), (96, 72, 32, 32, 4, 2, 1, 5, 33)]
IC_IDS = ["golden-size", "L33"]


CENTRED = lambda name: name.endswith(("ln.weight", "ln_msa.weight", "ln_pair.weight"))   # noqa: E731  drawn around 1
_restore_mode = G.restore_mode()


# ---- the forward, restated with the dropouts' keep maps (any floating type; differentiable) ---------------------------------------
def lin(P, name, x):
    y = x @ P[name + ".weight"].T
    return y + P[name + ".bias"] if name + ".bias" in P else y


def poswise(P, pre, x, H, keep=None, p=0.0):
    """O.poswise_weight with the dropout on the weights; also returns to_k's output (for the size of its gradient)"""
    B, N, L, d = x.shape
    dh = d // H
    q = lin(P, pre + ".to_q.0", x[:, 0]) * dh ** -0.5
    k = lin(P, pre + ".to_k.0", x)
    w = torch.einsum("blhc,bnlhc->bnhl", q.view(B, L, H, dh), k.view(B, N, L, H, dh)).softmax(1)
    if keep is not None:
        w = w * (keep.to(w.dtype) / (1.0 - p))
    return w.unsqueeze(-1), k


def block(P, pre, node, edge, H, keep=None, p=0.0):
    """O.graph_transformer_block with the dropout on the attention probabilities (keep [B, H, L, L])"""
    a = pre + ".attn"
    B, L, _ = node.shape
    q, k, v = (lin(P, f"{a}.node_to_{c}", node) for c in "qkv")
    HD = q.shape[-1]
    d = HD // H
    e = lin(P, a + ".edge_emb", edge).view(B, L, L, H, d)
    qh, kh, vh = q.view(B, L, H, d), k.view(B, L, H, d), v.view(B, L, H, d)
    att = ((torch.einsum("bihd,bjhd->bhij", qh, kh) + torch.einsum("bihd,bijhd->bhij", qh, e)) * d ** -0.5).softmax(-1)
    if keep is not None:
        att = att * (keep.to(att.dtype) / (1.0 - p))
    upd = (torch.einsum("bhij,bjhd->bihd", att, vh) + torch.einsum("bhij,bijhd->bihd", att, e)).reshape(B, L, HD)
    x = torch.nn.functional.layer_norm(lin(P, a + ".node_update", node) + upd, (HD,), P[pre + ".ln.weight"], P[pre + ".ln.bias"], 1e-5)
    return torch.nn.functional.elu(lin(P, pre + ".to_out.0", x)) + node


def coords(P, pre, msa, pair, onehot, aa_idx, n_layers, H, keeps=None, p=0.0):
    """O.initial_coord_generation with keeps = [the weights' keep map [B, N, 1, L], one [B, H, L, L] map per block]"""
    F = torch.nn.functional
    m = F.layer_norm(msa, msa.shape[-1:], P[pre + ".ln_msa.weight"], P[pre + ".ln_msa.bias"], 1e-5)
    w, _ = poswise(P, pre + ".poswise_weight", m, 1, None if keeps is None else keeps[0], p)
    node = F.elu(lin(P, pre + ".node_embed.0", torch.cat([(m * w[:, :, 0]).sum(1), onehot.to(msa.dtype)], -1)))
    dist = aa_idx.unsqueeze(-1) - aa_idx.unsqueeze(-2)
    sep = (torch.sign(dist) * torch.log(torch.abs(dist) + 1)).clamp(0.0, 5.5).unsqueeze(-1).to(msa.dtype)
    pn = F.layer_norm(pair, pair.shape[-1:], P[pre + ".ln_pair.weight"], P[pre + ".ln_pair.bias"], 1e-5)
    edge = F.elu(lin(P, pre + ".edge_embed.0", torch.cat([pn, sep], -1)))
    for i in range(n_layers):
        node = block(P, f"{pre}.blocks.{i}", node, edge, H, None if keeps is None else keeps[1 + i], p)
    return lin(P, pre + ".to_out", node).view(*node.shape[:2], 3, 3)


def check(got, ref, floor, dtype, tag, zero=None):
    """G.compare with every node_to_k.bias taken against its weight's gradient norm per input channel"""
    norms = {}
    for key in ref:
        if key.endswith("node_to_k.bias"):
            wref = ref[key[:-len("bias")] + "weight"]
            norms[key] = wref.norm().item() / wref.shape[1] ** 0.5
    G.compare(got, ref, dtype, tag, floor, zero=zero, norms=norms)


# ---- PositionWiseWeightFactor ----------------------------------------------------------------------------------------------------
def pw_make(d, H, p=0.0, seed=0):
    torch.manual_seed(200 + seed + d)
    return G.randomize(R.PositionWiseWeightFactor(d, H, p).to(DEV), 11 + seed, CENTRED)


def pw_inputs(d, H, N, L, dtype, seed):
    g_ = G.gen(seed)
    return torch.randn(2, N, L, d, generator=g_).to(dtype).float(), torch.randn(2, N, H, L, 1, generator=g_)


def pw_public(mod, x, w):
    got, out = G.grads_of(mod, {"x0": x}, w)
    return out, got["x0"]


def pw_check(mod, x, w, H, dtype, keep=None, p=0.0, dx=None, scale=1.0):
    """the gradients in mod's .grad (and dx) against the float64 autograd of the restatement"""
    P = G.state(mod)
    fn = lambda P, xx: poswise(P, "m", xx, H, keep, p)[0]  # noqa: E731
    ref, floor = G.oracle_grads(fn, P, {"x0": x}, w, UNIT[dtype], missing="zeros")
    got = dict({"m." + name: q.grad for name, q in mod.named_parameters()}, x0=dx)
    assert all(t is not None for t in got.values()), got
    got = {k: t.detach().double().cpu() / scale for k, t in got.items()}
    check(got, {k: v for k, v in ref.items() if k != "m.to_k.0.bias"}, floor, dtype, "poswise")
    # to_k.bias: an absolute bound, the size of the terms that cancel
    xx = x.double().cpu().requires_grad_()
    out, k = poswise(P, "m", xx, H, keep, p)
    k.retain_grad()
    (out * w.double()).sum().backward()
    size = k.grad.abs().sum((0, 1, 2)).norm().item()
    assert ref["m.to_k.0.bias"].norm().item() <= CEIL[dtype] * size            # the float64 reference's own rounding noise
    got = mod.to_k[0].bias.grad.double().cpu().norm().item() / scale
    print(f"to_k.0.bias: norm {got:.3e} against sum |dk| {size:.3e} (ceiling {CEIL[dtype] * size:.3e})")
    assert got <= CEIL[dtype] * size


def test_restatements_are_the_oracle():
    """the restatements used for the dropout cases are the oracle's functions where those apply (float64, CPU)"""
    d, H, N, L = PW_CASES[0]
    mod = pw_make(d, H)
    x = torch.randn(2, N, L, d, generator=G.gen(1), dtype=torch.float64)
    P = G.state(mod)
    torch.testing.assert_close(poswise(P, "m", x, H)[0], O.poswise_weight(P, "m", x, H), rtol=1e-12, atol=1e-14)
    cfg = IC_CASES[0]
    mod = ic_make(cfg)
    msa, pair, onehot, aa_idx, _ = ic_inputs(cfg, torch.float32, 3)
    P = G.state(mod)
    want = O.initial_coord_generation(P, "m", msa.double(), pair.double(), onehot.double(), aa_idx, cfg[5], cfg[4])
    torch.testing.assert_close(coords(P, "m", msa.double(), pair.double(), onehot, aa_idx, cfg[5], cfg[4]), want, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", PW_CASES, ids=str)
def test_poswise_grads_against_the_oracle(case, dtype):
    R.set_compute_dtype(dtype)
    d, H, N, L = case
    mod = pw_make(d, H).enable_backward()
    x, w = pw_inputs(d, H, N, L, dtype, 31 + L)
    twin = copy.deepcopy(mod).enable_backward(False)
    with torch.no_grad():
        plain = twin(x.to(DEV))
    out, dx = pw_public(mod, x, w)
    assert torch.equal(out, plain) and out.shape == (2, N, H, L, 1)      # recording leaves the forward's bits alone
    assert not twin(x.to(DEV).requires_grad_()).requires_grad           # the twin never records
    runs = [[dx.clone()] + [q.grad.clone() for q in mod.parameters()]]
    pw_check(mod, x, w, H, dtype, dx=dx)
    _, dx2 = pw_public(mod, x, w)                                       # the same bits on a second run
    assert all(torch.equal(a, b) for a, b in zip(runs[0], [dx2] + [q.grad for q in mod.parameters()]))


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_poswise_training_mode_replays_the_dropout(dtype):
    R.set_compute_dtype(dtype)
    d, H, N, L = PW_CASES[1]
    p, seed = 0.25, 77
    mod = pw_make(d, H, p, seed=1).enable_backward()
    x, w = pw_inputs(d, H, N, L, dtype, 41)
    with torch.no_grad():
        plain = mod(x.to(DEV))
    mod.train()
    R.manual_seed(seed)
    out, dx = pw_public(mod, x, w)
    assert not torch.equal(out, plain)    # the dropout acts
    assert RT.train_seed == seed and RT.train_offset == (2 * N * H * L + 3) // 4
    ones = torch.ones(2, N, H, L, device=DEV)
    keep = (ops.dropout(ones, p, seed, 0, out=torch.empty_like(ones)) != 0).cpu()
    pw_check(mod, x, w, H, dtype, keep, p, dx=dx)


def test_poswise_fp16_small_loss_does_not_underflow():
    R.set_compute_dtype(torch.float16)
    d, H, N, L = PW_CASES[0]
    mod = pw_make(d, H, seed=2).enable_backward()
    x, w = pw_inputs(d, H, N, L, torch.float16, 51)
    small = 1e-6
    _, dx = pw_public(mod, x, w * small)
    for t in [dx] + [q.grad for q in mod.parameters()]:
        assert torch.isfinite(t).all()
    assert dx.abs().max() > 0 and mod.to_k[0].weight.grad.abs().max() > 0
    pw_check(mod, x, w, H, torch.float16, dx=dx, scale=small)


def test_poswise_channel_count_must_be_a_multiple_of_8_when_recording():
    R.set_compute_dtype(torch.float32)
    mod = R.PositionWiseWeightFactor(12, 3, 0.0).to(DEV)
    x = torch.randn(1, 3, 5, 12, device=DEV)
    plain = mod(x.clone().requires_grad_())      # not opted in: nothing records, nothing to refuse
    assert not plain.requires_grad
    mod.enable_backward()
    with torch.no_grad():
        assert torch.equal(mod(x), plain)
    with pytest.raises(ValueError):
        mod(x.clone().requires_grad_())


# ---- InitialCoordGenerationWithMsaAndPair ------------------------------------------------------------------------------------------
def ic_make(cfg, p=0.0, seed=0):
    d_msa, d_pair, d_node, d_edge, H, layers = cfg[:6]
    torch.manual_seed(300 + seed + d_msa)
    return G.randomize(R.InitialCoordGenerationWithMsaAndPair(d_msa, d_pair, d_node, d_edge, H, layers, p).to(DEV), 13 + seed,
                       CENTRED)


def ic_inputs(cfg, dtype, seed):
    d_msa, d_pair, _, _, _, _, B, N, L = cfg
    g_ = G.gen(seed)
    msa = torch.randn(B, N, L, d_msa, generator=g_).to(dtype).float()
    pair = torch.randn(B, L, L, d_pair, generator=g_).to(dtype).float()
    onehot = torch.nn.functional.one_hot(torch.randint(0, 21, (B, L), generator=g_), 21).float()
    aa_idx = torch.arange(L).unsqueeze(0).repeat(B, 1)
    aa_idx[:, L // 2:] += 3      # a chain break: the sequence-separation column is not a plain ramp
    return msa, pair, onehot, aa_idx, torch.randn(B, L, 3, 3, generator=g_)


def ic_public(mod, msa, pair, onehot, aa_idx, w):
    got, out = G.grads_of(mod, {"x0": msa, "x1": pair, "onehot": onehot, "aa_idx": aa_idx}, w)
    assert got["onehot"] is None      # seq_onehot carries no gradient
    return out, got["x0"], got["x1"]


def ic_check(mod, cfg, ins, dtype, grads, keeps=None, p=0.0, scale=1.0):
    msa, pair, onehot, aa_idx, w = ins
    fn = lambda P, m_, p_: coords(P, "m", m_, p_, onehot.double(), aa_idx, cfg[5], cfg[4], keeps, p)  # noqa: E731
    ref, floor = G.oracle_grads(fn, G.state(mod), {"x0": msa, "x1": pair}, w, UNIT[dtype], missing="zeros")
    names = [n for n, _ in mod.named_parameters()]
    assert len(names) == len(set(names)) == len(list(mod.parameters()))
    got = dict({"m." + name: q.grad for name, q in mod.named_parameters()}, x0=grads[0], x1=grads[1])
    assert all(t is not None for t in got.values()), got
    got = {k: t.detach().double().cpu() / scale for k, t in got.items()}
    # poswise_weight.to_k.0.bias is constant over the MSA depth: exactly zero, not rounding noise (the oracle's own value is not held)
    check(got, ref, floor, dtype, "coords", zero={"m.poswise_weight.to_k.0.bias": float("inf")})


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("cfg", IC_CASES, ids=IC_IDS)
def test_coord_grads_against_the_oracle(cfg, dtype):
    R.set_compute_dtype(dtype)
    mod = ic_make(cfg).enable_backward()
    ins = ic_inputs(cfg, dtype, 61 + cfg[8])
    twin = copy.deepcopy(mod).enable_backward(False)
    assert not twin._rf_backward and not twin.blocks[0].attn._rf_backward and mod.blocks[1].attn._rf_backward
    dev_ins = [t.to(DEV) for t in ins[:4]]
    with torch.no_grad():
        plain = twin(*dev_ins)
        assert torch.equal(mod(*dev_ins), plain)
    assert not twin(dev_ins[0].clone().requires_grad_(), *dev_ins[1:]).requires_grad      # the twin never records
    out, dmsa, dpair = ic_public(mod, *ins)
    assert torch.equal(out, plain) and out.shape == (cfg[6], cfg[8], 3, 3)     # recording leaves the forward's bits alone
    first = [dmsa.clone(), dpair.clone()] + [q.grad.clone() for q in mod.parameters()]
    ic_check(mod, cfg, ins, dtype, (dmsa, dpair))
    _, dmsa2, dpair2 = ic_public(mod, *ins)                                     # the same bits on a second run
    assert all(torch.equal(a, b) for a, b in zip(first, [dmsa2, dpair2] + [q.grad for q in mod.parameters()]))


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_coord_training_mode_replays_both_dropouts(dtype):
    R.set_compute_dtype(dtype)
    cfg = IC_CASES[0]
    _, _, _, _, H, layers, B, N, L = cfg
    p, seed = 0.25, 91
    mod = ic_make(cfg, p, seed=1).enable_backward()
    ins = ic_inputs(cfg, dtype, 71)
    with torch.no_grad():
        plain = mod(*[t.to(DEV) for t in ins[:4]])
    mod.train()
    runs = []
    for _ in range(2):
        R.manual_seed(seed)
        out, dmsa, dpair = ic_public(mod, *ins)
        runs.append([out, dmsa.clone(), dpair.clone()] + [q.grad.clone() for q in mod.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert not torch.equal(runs[0][0], plain)    # the dropouts act
    # the forward's dropouts take the counters from 0 on (R.manual_seed): the weights' map first, then one map per block
    sizes = [(B, N, 1, L)] + [(B, H, L, L)] * layers
    keeps, off = [], 0
    for shape in sizes:
        ones = torch.ones(shape, device=DEV)
        keeps.append((ops.dropout(ones, p, seed, off, out=torch.empty_like(ones)) != 0).cpu())
        off += (ones.numel() + 3) // 4
    assert RT.train_seed == seed and RT.train_offset == off
    ic_check(mod, cfg, ins, dtype, runs[0][1:3], keeps, p)


def test_coord_fp16_small_loss_does_not_underflow():
    R.set_compute_dtype(torch.float16)
    cfg = IC_CASES[0]
    mod = ic_make(cfg, seed=2).enable_backward()
    msa, pair, onehot, aa_idx, w = ic_inputs(cfg, torch.float16, 81)
    small = 1e-6
    _, dmsa, dpair = ic_public(mod, msa, pair, onehot, aa_idx, w * small)
    for name, t in [("msa", dmsa), ("pair", dpair)] + [(n, q.grad) for n, q in mod.named_parameters()]:
        assert torch.isfinite(t).all(), name
        assert t.abs().max() > 0 or name == "poswise_weight.to_k.0.bias", name
    ic_check(mod, cfg, (msa, pair, onehot, aa_idx, w), torch.float16, (dmsa, dpair), scale=small)


def test_coord_channel_counts_must_be_multiples_of_8_when_recording():
    R.set_compute_dtype(torch.float32)
    mod = R.InitialCoordGenerationWithMsaAndPair(12, 16, 8, 8, 4, 1, 0.0).to(DEV)
    msa, pair = torch.randn(1, 3, 5, 12, device=DEV), torch.randn(1, 5, 5, 16, device=DEV)
    onehot, aa_idx = torch.zeros(1, 5, 21, device=DEV), torch.arange(5, device=DEV)[None]
    plain = mod(msa.clone().requires_grad_(), pair, onehot, aa_idx)
    assert not plain.requires_grad
    mod.enable_backward()
    with torch.no_grad():
        assert torch.equal(mod(msa, pair, onehot, aa_idx), plain)
    with pytest.raises(ValueError):
        mod(msa.clone().requires_grad_(), pair, onehot, aa_idx)


def test_full_model_forward_records_nothing_here():
    """RoseTTAFold.forward composes the module through run() without a tape: opted in, it computes the same bits and its
    coordinates carry no autograd history"""
    R.set_compute_dtype(torch.bfloat16)
    cfg = dict(d_input=21, d_msa=96, d_pair=72, d_node=8, d_edge=8, d_state=8, n_two_track_blocks=1, n_three_track_blocks=1,
               n_encoder_layers=1, max_len=64, n_neighbors=[128], p_dropout=0.0)
    torch.manual_seed(1234)
    model = R.RoseTTAFold(**cfg).to(DEV)
    g_ = G.gen(0)
    msa = torch.randint(0, 21, (1, 8, 16), generator=g_)
    args = (msa.to(DEV), msa[:, 0].clone().to(DEV), torch.arange(16).unsqueeze(0).to(DEV))
    with torch.no_grad():
        want = model(*args)
    ic = model.initial_coord_generation_with_msa_and_pair.enable_backward()
    assert ic._rf_backward and all(b._rf_backward and b.attn._rf_backward for b in ic.blocks)
    logits, xyz, plddt = model(*args)      # grad mode on
    assert not xyz.requires_grad and xyz.grad_fn is None
    assert torch.equal(xyz, want[1]) and torch.equal(logits["dist"], want[0]["dist"]) and torch.equal(plddt, want[2])
