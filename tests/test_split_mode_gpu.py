"""The float32 compute mode under set_float32_matmul_precision("high") (split-bf16 GEMMs, RF_F32X3): modules and a 2+2-depth
forward against the CPU oracle, the full 8+5 depth against the exact float32 mode, hipGraph replay, and the way back to
"highest".  Accuracy targets: see the split-precision section of DESIGN.md."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import _lib as L  # noqa: E402
from rosettafold_pytorch_amd import ops  # noqa: E402
from oracle import rf_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import depth_parity as DP  # noqa: E402

DEV = "cuda"
B, N, Lr, DM, DPAIR = 2, 8, 16, 96, 72
TOL = 1e-3  # max-norm, relative to max |ref| (exact fp32 mode: 2e-4, fp16 mode: 6e-3 in test_modules_gpu.py)


@pytest.fixture
def high():
    R.set_compute_dtype(torch.float32)
    R.set_float32_matmul_precision("high")
    yield
    R.set_float32_matmul_precision("highest")
    R.set_compute_dtype(torch.bfloat16)


@pytest.fixture
def families(monkeypatch):
    """kernel family of every ops.gemm launch"""
    seen = []
    orig = ops.gemm

    def rec(*a, **k):
        out = orig(*a, **k)
        seen.append(L.lib.rf_gemm_last_family())
        return out
    monkeypatch.setattr(ops, "gemm", rec)
    return seen


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-20)).item()


def rn(*s, seed=0):
    return torch.randn(*s, generator=torch.Generator().manual_seed(seed + len(s) + sum(s)))


def state(mod):
    return {"m." + k: v.detach().float().cpu() for k, v in mod.state_dict().items()}


def build(ctor, seed=11):
    torch.manual_seed(seed)
    return ctor().to(DEV)


def test_tied_encoder_layer(high, families):
    m = build(lambda: R.EncoderLayer(d_msa=DM, d_ff=4 * DM, n_heads=12, p_dropout=0.0, tied=True, return_att=True))
    x = rn(B, N, Lr, DM)
    out, att = m(x.to(DEV))
    ro, ra = O.encoder_layer_tied(state(m), "m", x, 12)
    assert rel(out, ro) < TOL and rel(att, ra) < TOL, (rel(out, ro), rel(att, ra))
    assert 5 in families and 0 not in families, families


def test_pair_update_with_msa_conv_path(high, families):
    m = build(lambda: R.PairUpdateWithMsa(d_msa=DM, d_proj=32, d_pair=DPAIR, n_heads=12, p_dropout=0.0))
    msa, pair, att = rn(B, N, Lr, DM), rn(B, Lr, Lr, DPAIR), torch.rand(B, Lr, Lr, 12)
    got = m(msa.to(DEV), pair.to(DEV), att.to(DEV))
    e = rel(got, O.pair_update_with_msa(state(m), "m", msa, pair, att))
    assert e < TOL, e
    assert 5 in families and 0 not in families, families


def test_prediction_head(high, families):
    m = build(lambda: R.PredictionHead(DPAIR, 4, 0.0))
    pair = rn(B, Lr, Lr, DPAIR)
    out = m(pair.to(DEV))
    ref = O.prediction_head(state(m), "m", pair, 4)
    for k in ("theta", "phi", "dist", "omega"):
        assert rel(out[k], ref[k]) < TOL, (k, rel(out[k], ref[k]))
    assert 5 in families and 0 not in families, families


class _Args:
    oracle, struct_lowp, modes, B, N, L, n_two, n_three = True, False, "fp32x3", 1, 128, 256, 2, 2


def test_depth_2_2_against_the_oracle():
    r = DP.run(_Args())
    assert R.get_float32_matmul_precision() == "highest" and R.model.T() == torch.bfloat16  # the tool restores both
    x = r["fp32x3"]
    print("\n[depth fp32x3 vs oracle]", x["rel_l2"], x["dist_argmax_agreement"], x["dist_argmax_agreement_clear_margin"])
    print("[curve]", x["curve"])
    for k in ("theta", "phi", "dist", "omega"):
        assert x["rel_l2"][k] < 1e-3, (k, x["rel_l2"])
    assert x["rel_l2"]["xyz"] < 2e-2, x["rel_l2"]
    assert x["dist_argmax_agreement"] >= 0.9995
    assert x["dist_argmax_agreement_clear_margin"] == 1.0


class _ArgsFull:
    oracle, struct_lowp, modes, B, N, L, n_two, n_three = False, False, "fp32x3", 1, 128, 256, 8, 5


def test_full_depth_against_the_exact_mode():
    r = DP.run(_ArgsFull())
    x = r["fp32x3"]
    print("\n[depth 8+5 fp32x3 vs exact fp32]", x["rel_l2"], x["dist_argmax_agreement"])
    print("[curve]", x["curve"])
    for k in ("theta", "phi", "dist", "omega"):
        assert x["rel_l2"][k] < 2e-3, (k, x["rel_l2"])
    assert x["dist_argmax_agreement"] >= 0.999


CFG = dict(d_input=21, d_msa=DM, d_pair=DPAIR, d_node=8, d_edge=8, d_state=8, n_two_track_blocks=1, n_three_track_blocks=2,
           n_encoder_layers=1, max_len=64, n_neighbors=[128, 128], p_dropout=0.0)


def _inputs():
    g = torch.Generator().manual_seed(0)
    msa = torch.randint(0, 21, (B, N, Lr), generator=g)
    return msa.to(DEV), msa[:, 0].clone().to(DEV), torch.arange(Lr).unsqueeze(0).repeat(B, 1).to(DEV)


def test_graphed_forward_and_precision_switch():
    model = build(lambda: R.RoseTTAFold(**CFG)).eval()
    msa, seq, aa = _inputs()
    try:
        R.set_compute_dtype(torch.float32)
        with torch.no_grad():
            exact = [t.clone() for t in _flat(model(msa, seq, aa))]
        R.set_float32_matmul_precision("high")
        with torch.no_grad():
            eager = [t.clone() for t in _flat(model(msa, seq, aa))]
        assert any(not torch.equal(a, b) for a, b in zip(eager, exact))  # the split kernel ran
        g = R.GraphedForward(model, msa, seq, aa)
        replay = [t.clone() for t in _flat(g(msa, seq, aa))]
        for a, b in zip(replay, eager):
            assert torch.equal(a, b)
        R.set_float32_matmul_precision("highest")
        with pytest.raises(L.RfmiError):
            g(msa, seq, aa)
        g.recapture()
        for a, b in zip(_flat(g(msa, seq, aa)), exact):
            assert torch.equal(a, b)
        with torch.no_grad():
            back = _flat(model(msa, seq, aa))
        for a, b in zip(back, exact):  # "highest" after "high" is the exact mode, bit for bit
            assert torch.equal(a, b)
    finally:
        R.set_float32_matmul_precision("highest")
        R.set_compute_dtype(torch.bfloat16)


def _flat(out):
    logits, xyz, plddt = out
    return [logits[k] for k in sorted(logits)] + [xyz, plddt]
