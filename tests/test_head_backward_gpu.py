"""Backward pass of PredictionHead / ResNet / ResBlock2D (enable_backward): the three new kernels against float64 CPU autograd,
the modules' gradients against the CPU oracle (torch autograd through oracle/rf_oracle.py) in the three compute modes, dropout
replay in training mode (finite differences), the fp16 gradient scaling, unchanged forward numbers, determinism, and the full
model with a trainable head.

The references come from tests/grad_oracle.py (oracle_grads with one weight tensor per output).  The comparison is this file's
own `compare`: the mode's ceiling with `<=` (the ELUs are smooth: no kink floor), and an absolute bound for the two biases that
are exactly zero in exact arithmetic."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import grad_oracle as G  # noqa: E402
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import ops  # noqa: E402
from oracle import rf_oracle as O  # noqa: E402

DEV = "cuda"
MODES, CEIL = G.MODES, G.CEIL
_restore_mode = G.restore_mode()


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("C,taps,dil,L,Co", [(64, 9, 1, 40, 64), (64, 9, 2, 40, 64), (64, 9, 4, 40, 64), (64, 9, 8, 40, 64),
                                             (288, 9, 1, 40, 288), (288, 9, 8, 24, 288), (288, 1, 1, 40, 40),
                                             (288, 1, 1, 40, 24), (64, 1, 1, 40, 288), (64, 1, 1, 37, 64)])
def test_conv_wgrad_against_cpu(dtype, C, taps, dil, L, Co):
    R.set_compute_dtype(dtype)
    g = G.gen(C + taps + dil + L + Co)
    B = 2
    x = torch.randn(B, L, L, C, generator=g).to(dtype)
    dy = torch.randn(B, L, L, Co, generator=g).to(dtype)
    dw, db = ops.conv_wgrad(dy.to(DEV), x.to(DEV), taps, dil, bias=True)
    k = 3 if taps == 9 else 1
    ref = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (Co, C, k, k), dy.double().permute(0, 3, 1, 2),
                                      padding=dil if taps == 9 else 0, dilation=dil)
    ref = ref.permute(0, 2, 3, 1).reshape(Co, taps * C)   # the forward's [co][tap][ci] layout
    assert G.rel(dw, ref) < 1e-5
    assert G.rel(db, dy.double().sum((0, 1, 2))) < 1e-5
    dw2, db2 = ops.conv_wgrad(dy.to(DEV), x.to(DEV), taps, dil, bias=True)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("act", [False, True])
def test_instnorm_bwd_against_cpu(dtype, act):
    R.set_compute_dtype(dtype)
    g = G.gen(7 + act)
    B, L, C = 2, 40, 64
    x = (torch.randn(B, L, L, C, generator=g) * 2 + 0.5).to(dtype)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.1
    gy = torch.randn(B, L, L, C, generator=g)
    xd = x.double().permute(0, 3, 1, 2).requires_grad_()
    gd, bd = gamma.double().requires_grad_(), beta.double().requires_grad_()
    y = F.instance_norm(xd, weight=gd, bias=bd, eps=1e-6)
    if act:
        y = F.elu(y)
    (y * gy.double().permute(0, 3, 1, 2)).sum().backward()
    stats = []
    xg = x.to(DEV)
    ops.instnorm(xg, gamma.to(DEV), beta.to(DEV), eps=1e-6, out_dtype=torch.float32, stats_out=stats)
    a = y.detach().permute(0, 2, 3, 1).float().contiguous().to(DEV) if act else None
    dx, dgam, dbet = ops.instnorm_bwd(gy.to(DEV), xg, stats[0], gamma.to(DEV), eps=1e-6, act_out=a, dx_dtype=R.T())
    tol = {torch.float32: 1e-4, torch.bfloat16: 8e-3, torch.float16: 1e-3}[dtype]
    assert G.rel(dx, xd.grad.permute(0, 2, 3, 1)) < tol
    assert G.rel(dgam, gd.grad) < 1e-4 and G.rel(dbet, bd.grad) < 1e-4
    dx2, dgam2, dbet2 = ops.instnorm_bwd(gy.to(DEV), xg, stats[0], gamma.to(DEV), eps=1e-6, act_out=a, dx_dtype=R.T())
    assert torch.equal(dx, dx2) and torch.equal(dgam, dgam2) and torch.equal(dbet, dbet2)


@pytest.mark.parametrize("D", [64, 288])
def test_layernorm_bwd_against_cpu(D):
    g = G.gen(D)
    x = torch.randn(3, 40, 40, D, generator=g) * 3 + 1
    gamma, beta = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)
    gy = torch.randn(3, 40, 40, D, generator=g)
    xd = x.double().requires_grad_()
    gd, bd = gamma.double().requires_grad_(), beta.double().requires_grad_()
    (F.layer_norm(xd, (D,), gd, bd, 1e-5) * gy.double()).sum().backward()
    dx, dgam, dbet = ops.layernorm_bwd(x.to(DEV), gy.to(DEV), gamma.to(DEV), eps=1e-5)
    assert G.rel(dx, xd.grad) < 1e-5 and G.rel(dgam, gd.grad) < 1e-5 and G.rel(dbet, bd.grad) < 1e-5
    dx2, dgam2, dbet2 = ops.layernorm_bwd(x.to(DEV), gy.to(DEV), gamma.to(DEV), eps=1e-5)
    assert torch.equal(dx, dx2) and torch.equal(dgam, dgam2) and torch.equal(dbet, dbet2)


# ------------------------------------------------------------------------------------------------ modules vs oracle
def _init_affine(mod, seed):
    """non-trivial InstanceNorm / LayerNorm affine parameters (the default 1 / 0 would hide a swapped gamma / beta)"""
    g = G.gen(seed)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, (torch.nn.InstanceNorm2d, torch.nn.LayerNorm)):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)


def outputs(out):
    return out if isinstance(out, dict) else {"out": out}


def reference(fn, mod, pre, inp, R_):
    """({parameter name: float64 gradient}, the input's) of sum_k sum(fn(P, x)[k] * R_[k])"""
    ref, _ = G.oracle_grads(fn, G.state(mod, pre), {"x": inp},
                            lambda out: sum((o * R_[k].double()).sum() for k, o in outputs(out).items()))
    return {k[len(pre) + 1:]: v for k, v in ref.items() if k != "x"}, ref["x"]


def module_grads(mod, inp, R_):
    def loss(out):
        assert all(o.requires_grad for o in outputs(out).values())
        return sum((o * R_[k].to(DEV)).sum() for k, o in outputs(out).items())
    got, out = G.grads_of(mod, {"x": inp}, loss, pre="")
    return {k[1:]: v for k, v in got.items() if k != "x"}, got["x"], outputs(out)


def compare(dtype, got, ref, gx, rx, zero_keys=()):
    ceil = CEIL[dtype]
    errs = {}
    for k, r in ref.items():
        assert got[k] is not None, k
        assert torch.isfinite(got[k]).all(), k
        if k in zero_keys:   # exactly zero in exact arithmetic: an absolute bound scaled by the matching weight's gradient
            continue
        errs[k] = G.rel(got[k], r)
    errs["input"] = G.rel(gx, rx)
    bad = {k: e for k, e in errs.items() if e > ceil}
    print(f"{dtype} max rel-L2 {max(errs.values()):.3e} ({max(errs, key=errs.get)})")
    assert not bad, bad
    for k in zero_keys:
        wk = k.replace(".bias", ".weight")
        assert got[k].double().norm().item() <= ceil * got[wk].double().norm().item() + 1e-12, k


@pytest.mark.parametrize("dtype", MODES)
def test_resblock2d_against_oracle(dtype):
    R.set_compute_dtype(dtype)
    torch.manual_seed(1)
    mod = R.ResBlock2D(64, 3, 2).to(DEV).enable_backward()
    _init_affine(mod, 1)
    x = torch.randn(2, 64, 40, 40, generator=G.gen(2))
    R_ = {"out": torch.randn(2, 64, 40, 40, generator=G.gen(3))}
    got, gx, _ = module_grads(mod, x, R_)
    ref, rx = reference(lambda P, x: O.resblock2d(P, "m", x, 2), mod, "m", x, R_)
    compare(dtype, got, ref, gx, rx)


@pytest.mark.parametrize("dtype", MODES)
def test_resnet_against_oracle(dtype):
    R.set_compute_dtype(dtype)
    torch.manual_seed(2)
    mod = R.ResNet(4, 64, 64, 37).to(DEV).enable_backward()
    _init_affine(mod, 2)
    x = torch.randn(2, 64, 40, 40, generator=G.gen(4))
    R_ = {"out": torch.randn(2, 37, 40, 40, generator=G.gen(5))}
    got, gx, _ = module_grads(mod, x, R_)
    ref, rx = reference(lambda P, x: O.resnet(P, "m", x, 4), mod, "m", x, R_)
    compare(dtype, got, ref, gx, rx)


def head_case(seed=3, C=64, B=2, L=40):
    torch.manual_seed(seed)
    head = R.PredictionHead(C, 4, 0.15).to(DEV)
    _init_affine(head, seed)
    pair = torch.randn(B, L, L, C, generator=G.gen(seed)) + 0.3
    R_ = {k: torch.randn(B, L, L, 19 if k == "phi" else 37, generator=G.gen(seed + i)) for i, k in enumerate(("theta", "phi", "dist", "omega"))}
    return head, pair, R_


@pytest.mark.parametrize("dtype", MODES)
def test_prediction_head_against_oracle(dtype):
    R.set_compute_dtype(dtype)
    head, pair, R_ = head_case()
    head.enable_backward()
    got, gx, _ = module_grads(head, pair, R_)
    ref, rx = reference(lambda P, x: O.prediction_head(P, "h", x, 4), head, "h", pair, R_)
    # LayerNorm beta and the projection bias: exactly zero (every consumer starts bias-free 1x1 conv -> InstanceNorm)
    compare(dtype, got, ref, gx, rx, zero_keys=("proj.0.bias", "proj.1.bias"))


@functools.lru_cache(maxsize=1)
def _production_case():
    torch.manual_seed(5)
    mod = R.ResNet(4, 288, 288, 37)
    _init_affine(mod, 5)
    x = torch.randn(1, 288, 256, 256, generator=G.gen(6))
    R_ = {"out": torch.randn(1, 37, 256, 256, generator=G.gen(7))}
    P = {"m." + k: v.detach().float().requires_grad_() for k, v in mod.state_dict().items()}
    xr = x.clone().requires_grad_()
    (O.resnet(P, "m", xr, 4) * R_["out"]).sum().backward()
    return mod, x, R_, {k[2:]: v.grad.double() for k, v in P.items()}, xr.grad.double()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_resnet_production_shape_against_oracle(dtype):
    """one ResNet(4, 288, 288, 37) at B = 1, L = 256: the conv288 input-gradient path and full-width weight-gradient tiles"""
    R.set_compute_dtype(dtype)
    mod, x, R_, ref, rx = _production_case()
    mod = mod.to(DEV).enable_backward()
    got, gx, _ = module_grads(mod, x, R_)
    compare(dtype, got, ref, gx, rx)


# ------------------------------------------------------------------------------------------------ training mode, fp16 scale
def test_training_mode_finite_difference():
    R.set_compute_dtype(torch.float32)
    head, pair, R_ = head_case(seed=11, C=32, L=24)
    head.train().enable_backward()
    pd = pair.to(DEV)

    def loss():
        R.manual_seed(77)
        out = head(pd)
        return sum((out[k].double() * R_[k].to(DEV).double()).sum() for k in out)

    for p in head.parameters():
        p.grad = None
    loss().backward()
    v = [torch.randn(p.shape, generator=G.gen(i)).to(DEV) for i, p in enumerate(head.parameters())]
    dot = sum((p.grad * vi).sum() for p, vi in zip(head.parameters(), v)).item()
    eps = 1e-4   # (1e-3 leaves a 5e-2 curvature term across the ELUs)
    with torch.no_grad():
        for p, vi in zip(head.parameters(), v):
            p.add_(eps * vi)
        lp = loss().item()
        for p, vi in zip(head.parameters(), v):
            p.sub_(2 * eps * vi)
        lm = loss().item()
        for p, vi in zip(head.parameters(), v):
            p.add_(eps * vi)
    fd = (lp - lm) / (2 * eps)
    assert abs(fd - dot) <= 1e-2 * abs(dot), (fd, dot)


def test_fp16_small_loss_does_not_underflow():
    R.set_compute_dtype(torch.float16)
    head, pair, R_ = head_case(seed=13)
    head.enable_backward()
    g1, x1, _ = module_grads(head, pair, R_)
    g1 = {k: v.clone() for k, v in g1.items()}
    g2, x2, _ = module_grads(head, pair, {k: v * 1e-6 for k, v in R_.items()})
    for k in g1:
        if k not in ("proj.0.bias", "proj.1.bias"):
            assert G.rel(g2[k] * 1e6, g1[k]) < CEIL[torch.float16], k
    assert G.rel(x2 * 1e6, x1) < CEIL[torch.float16]


# ------------------------------------------------------------------------------------------------ forward, determinism, errors
@pytest.mark.parametrize("dtype", MODES)
def test_recording_forward_is_bitwise_unchanged(dtype):
    R.set_compute_dtype(dtype)
    head, pair, _ = head_case(seed=17)
    pd = pair.to(DEV)
    plain = head(pd)
    assert not any(o.requires_grad for o in plain.values())
    head.enable_backward()
    with torch.no_grad():
        off = head(pd)
    rec = head(pd)
    assert all(o.requires_grad for o in rec.values())
    for k in plain:
        assert torch.equal(plain[k], rec[k].detach()) and torch.equal(plain[k], off[k])


@pytest.mark.parametrize("dtype", MODES)
def test_backward_is_deterministic(dtype):
    R.set_compute_dtype(dtype)
    head, pair, R_ = head_case(seed=19)
    head.enable_backward()
    g1, x1, _ = module_grads(head, pair, R_)
    g1 = {k: v.clone() for k, v in g1.items()}
    g2, x2, _ = module_grads(head, pair, R_)
    assert torch.equal(x1, x2) and all(torch.equal(g1[k], g2[k]) for k in g1)


def test_row_sharded_call_with_backward_raises():
    head, pair, _ = head_case(seed=23)
    head.enable_backward()
    with pytest.raises(NotImplementedError):
        head.run(pair.to(DEV), row_group=object())


def test_channel_counts_the_backward_does_not_take_raise():
    mod = R.ResNet(1, 12, 12, 5).to(DEV).enable_backward()
    with pytest.raises(ValueError):
        mod(torch.randn(1, 12, 8, 8, device=DEV))


CFG1 = dict(d_msa=96, d_pair=64, d_node=8, d_edge=8, d_state=8, n_two_track_blocks=1, n_three_track_blocks=2,
            n_encoder_layers=1, max_len=64, n_neighbors=[128, 128])


def test_full_model_trains_the_head():
    R.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(29)
    model = R.RoseTTAFold(**CFG1).to(DEV)
    model.prediction_head.enable_backward()
    g = G.gen(31)
    B, N, L = 1, 8, 48
    msa = torch.randint(0, 21, (B, N, L), generator=g).to(DEV)
    seq, idx = msa[:, 0].clone(), torch.arange(L).repeat(B, 1).to(DEV)
    bins = torch.randint(0, 37, (B, L, L), generator=g).to(DEV)
    head_params = set(model.prediction_head.parameters())
    opt = torch.optim.SGD(model.prediction_head.parameters(), lr=2e-3)
    losses = []
    for step in range(6):
        opt.zero_grad()
        logits, xyz, plddt = model(msa, seq, idx)
        assert logits["dist"].requires_grad and not xyz.requires_grad and not plddt.requires_grad
        loss = F.cross_entropy(logits["dist"].reshape(-1, 37), bins.reshape(-1))
        loss.backward()
        losses.append(loss.item())
        if step == 0:
            assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in head_params)
            assert all(p.grad is None for p in model.parameters() if p not in head_params)
        if step < 5:
            with torch.no_grad():
                before = model(msa, seq, idx)[0]["dist"].clone()
            opt.step()
            with torch.no_grad():
                after = model(msa, seq, idx)[0]["dist"]
            assert not torch.equal(before, after)   # the next forward sees the new weights (cache invalidation)
    assert losses[5] < losses[0], losses
    gf = R.GraphedForward(model, msa, seq, idx)
    assert not gf(msa, seq, idx)[0]["dist"].requires_grad
