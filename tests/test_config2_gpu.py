"""GPU parity at the BENCHMARK dimensions (BASELINE.json configs[1]: N=128, L=256, d_msa=384, d_pair=288, 12/8/4 heads,
d_node=d_edge=d_state=32, k=128) -- one layer of each kind of the forward path against the CPU oracle on one sample
(samples are independent), in BOTH compute modes.  At these shapes the model takes the fused kernels the
bench times (persistent GEMM, fused FAVOR+, fused tied attention, fused outer product): this is the composition the
small-dimension module tests never reach.  Plus one pair-axial layer at configs[3] size (L=1024).

Stated tolerances (max |a-b| / max |ref|, and relative L2):
  fp32 mode (exact fp32 tiles)            2e-5 / 2e-5      (observed <= 2.1e-6 / 2.0e-6)
  bf16 mode (MFMA, fp32 accumulate)       2e-2 / 1.5e-2    (observed <= 8.3e-3 / 7.6e-3)
  fp16 mode (MFMA f16, librfmi_f16.so)    4e-3 / 3e-3      (the same kernels built with IEEE fp16 operands: 8x less rounding)
"""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import rosettafold_pytorch_amd as R  # noqa: E402
from oracle import rf_oracle as O  # noqa: E402

DEV = "cuda"
N2, L2, DM, DP, DN, DE, DS = 128, 256, 384, 288, 32, 32, 32
TOL = {torch.float32: (2e-5, 2e-5), torch.bfloat16: (2e-2, 1.5e-2), torch.float16: (4e-3, 3e-3)}


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-20)).item()


def rel2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def rn(*s, seed=0):
    return torch.randn(*s, generator=torch.Generator().manual_seed(seed + len(s) + sum(s)))


def state(mod, prefix="m"):
    return {prefix + "." + k: v.detach().float().cpu() for k, v in mod.state_dict().items()}


def build(ctor, seed=11):
    torch.manual_seed(seed)
    return ctor().to(DEV)


def xyz_trace(b, l, seed=3):
    g = torch.Generator().manual_seed(seed)
    steps = torch.randn(b, l, 3, generator=g)
    ca = torch.cumsum(3.8 * steps / steps.norm(dim=-1, keepdim=True), 1)
    xyz = ca[:, :, None, :] + 0.5 * torch.randn(b, l, 3, 3, generator=g)
    xyz[:, :, 1] = ca
    return xyz


@pytest.fixture(params=[torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def mode(request):
    R.set_compute_dtype(request.param)
    yield request.param
    R.set_compute_dtype(torch.bfloat16)


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    torch.set_num_threads(min(16, torch.get_num_threads() or 16))
    yield


def check(name, mode, got, ref, loose=None):
    tmax, tl2 = TOL[mode] if loose is None else loose
    e, e2 = rel(got, ref), rel2(got, ref)
    print(f"\n[config2 {name} {str(mode).split('.')[-1]}] max-rel {e:.3e}  rel-L2 {e2:.3e}")
    assert e < tmax and e2 < tl2, (name, e, e2)


def test_tied_row_layer(mode):
    m = build(lambda: R.EncoderLayer(d_msa=DM, d_ff=4 * DM, n_heads=12, p_dropout=0.0, tied=True, return_att=True))
    x = rn(1, N2, L2, DM)
    out, att = m(x.to(DEV))
    ro, ra = O.encoder_layer_tied(state(m), "m", x, 12)
    check("tied_row_layer.out", mode, out, ro)
    check("tied_row_layer.att", mode, att, ra)
    assert torch.equal(att, att.transpose(1, 2))


def test_performer_column_layer(mode):
    # the model runs the column layers on [B, N, L, D] with the sequences along the MSA depth (seq_axis=1)
    m = build(lambda: R.EncoderLayer(d_msa=DM, d_ff=4 * DM, n_heads=12, p_dropout=0.0, tied=False, performer=True))
    x = rn(1, N2, L2, DM)
    xd = x.to(DEV).clone()
    m.run(xd, seq_axis=1)
    ref = O.encoder_layer_performer(state(m), "m", x.transpose(1, 2).contiguous(), 12).transpose(1, 2)
    check("performer_column_layer", mode, xd, ref)


def test_pair_update_with_msa(mode):
    m = build(lambda: R.PairUpdateWithMsa(d_msa=DM, d_proj=32, d_pair=DP, n_heads=12, p_dropout=0.0))
    msa, pair = rn(1, N2, L2, DM), rn(1, L2, L2, DP)
    att = torch.rand(1, L2, L2, 12, generator=torch.Generator().manual_seed(2)).softmax(2)
    got = m(msa.to(DEV), pair.to(DEV), att.to(DEV))
    check("pair_update_with_msa", mode, got, O.pair_update_with_msa(state(m), "m", msa, pair, att))


def test_outer_product_mean(mode):
    m = build(lambda: R.OuterProductMean(32, DP))
    xa, xb = rn(1, N2, L2, 32), rn(1, N2, L2, 32, seed=1) * 0.1
    check("outer_product_mean", mode, m(xa.to(DEV), xb.to(DEV)), O.outer_product_mean(state(m), "m", xa, xb))


def test_pair_axial_layer(mode):
    m = build(lambda: R.PairUpdateWithAxialAttentionLayer(DP, 4 * DP, 8, 0.0, {}))
    x = rn(1, L2, L2, DP)
    check("pair_axial_layer", mode, m(x.to(DEV)), O.pair_axial_layer(state(m), "m", x, 8))


def test_msa_update_with_pair_layer(mode):
    m = build(lambda: R.MsaUpdateWithPair(DM, DP, 4, n_encoder_layers=1, p_dropout=0.0))
    msa, pair = rn(1, N2, L2, DM), rn(1, L2, L2, DP)
    check("msa_update_with_pair_layer", mode, m(msa.to(DEV), pair.to(DEV)),
          O.msa_update_with_pair(state(m), "m", msa, pair, 1, 4))


def test_coord_update_k128(mode):
    m = build(lambda: R.CoordUpdateWithMsaAndPair(DM, DP, DN, DE, DS, n_neighbors=128, p_dropout=0.0))
    msa, pair, xyz = rn(1, N2, L2, DM), rn(1, L2, L2, DP), xyz_trace(1, L2)
    seq = torch.randint(0, 21, (1, L2), generator=torch.Generator().manual_seed(1))
    oh = torch.nn.functional.one_hot(seq, 21).float()
    aa = torch.arange(L2).unsqueeze(0)
    st, xo = m(xyz.to(DEV), msa.to(DEV), pair.to(DEV), aa.to(DEV), oh.to(DEV))
    rs, rx = O.coord_update(state(m), "m", xyz, msa, pair, aa, oh, 128, DS)
    # the structure track computes in fp32 in EVERY mode, including its node / edge inputs (RT.struct_inputs_fp32, round 3: the
    # 16-bit LayerNorm(msa) that used to feed the node features tripped the network's discontinuities -- GNormBias -- and needed a
    # 0.3 bound): the fp32 tolerance holds for all three modes (observed 2e-6 / 1e-7 in each)
    check("coord_update.state", mode, st, rs, TOL[torch.float32])
    check("coord_update.xyz", mode, xo, rx, TOL[torch.float32])


def test_msa_update_with_pair_and_coord(mode):
    m = build(lambda: R.MsaUpdateWithPairAndCoord(DM, DS, 32, 4 * DM, p_dropout=0.0))
    msa, st, xyz = rn(1, N2, L2, DM), rn(1, L2, DS), xyz_trace(1, L2)
    check("msa_update_with_pair_and_coord", mode, m(xyz.to(DEV), st.to(DEV), msa.to(DEV)),
          O.msa_update_with_pair_and_coord(state(m), "m", xyz, st, msa))


def test_prediction_head(mode):
    m = build(lambda: R.PredictionHead(DP, 4, 0.0))
    pair = rn(1, L2, L2, DP)
    out = m(pair.to(DEV))
    ref = O.prediction_head(state(m), "m", pair, 4)
    for k_ in ("theta", "phi", "dist", "omega"):
        check("prediction_head." + k_, mode, out[k_], ref[k_])
    agree = (out["dist"].argmax(-1).cpu() == ref["dist"].argmax(-1)).float().mean().item()
    print(f"[config2 prediction_head] distogram argmax agreement {agree:.5f}")
    if mode == torch.float32:
        assert agree == 1.0  # the strict claim: exact-fp32 mode reproduces every distogram bin


def _performer_chunked(P, pre, x, heads, chunk=32):
    """O.performer_self_attention over sequence batches (the features of 1024 x 1024-row sequences do not fit the host)."""
    return torch.cat([O.performer_self_attention(P, pre, x[i:i + chunk], heads, True) for i in range(0, x.shape[0], chunk)])


def test_pair_axial_layer_L1024_config4():
    """BASELINE.json configs[3]: L=1024 pair track (1.2 GB fp32 stream, chunked FAVOR+ kernel), bf16 path."""
    R.set_compute_dtype(torch.bfloat16)
    Ll = 1024
    m = build(lambda: R.PairUpdateWithAxialAttentionLayer(DP, 4 * DP, 8, 0.0, {}))
    x = rn(1, Ll, Ll, DP)
    got = m(x.to(DEV)).cpu()
    P = state(m)
    t0 = time.time()
    with torch.no_grad():
        xn = O._ln(P, "m.layer.0.fn.0", x)
        a = _performer_chunked(P, "m.row_attn", xn.permute(0, 2, 1, 3).reshape(Ll, Ll, DP), 8)
        y = x + a.view(1, Ll, Ll, DP).permute(0, 2, 1, 3)
        xn = O._ln(P, "m.layer.1.fn.0", y)
        y = y + _performer_chunked(P, "m.col_attn", xn.reshape(Ll, Ll, DP), 8).view(1, Ll, Ll, DP)
        ref = y + O.feed_forward(P, "m.ff", O._ln(P, "m.layer.2.fn.0", y))
    print(f"\n[config4 pair_axial_layer L=1024] oracle {time.time() - t0:.1f}s")
    check("pair_axial_layer_L1024", torch.bfloat16, got, ref)


def test_run_to_run_bitwise_config2():
    """Every layer kind at the BENCH dimensions twice on the same inputs: bitwise identical (a race or an uninitialised
    read in a hand-written kernel shows up here; tools/determinism_modules.py is the B=4 form of this check, and
    tools/determinism_favor.py the per-variant form for the fused FAVOR+ kernel, where round 2 found and fixed one)."""
    R.set_compute_dtype(torch.bfloat16)
    msa, pair = rn(1, N2, L2, DM).to(DEV), rn(1, L2, L2, DP).to(DEV)

    def twice(name, fn):
        a, b = fn(), fn()
        fa = [a[k] for k in sorted(a)] if isinstance(a, dict) else list(a) if isinstance(a, (tuple, list)) else [a]
        fb = [b[k] for k in sorted(b)] if isinstance(b, dict) else list(b) if isinstance(b, (tuple, list)) else [b]
        for x, y in zip(fa, fb):
            if torch.is_tensor(x):
                assert torch.equal(x, y), name

    m = build(lambda: R.EncoderLayer(d_msa=DM, d_ff=4 * DM, n_heads=12, p_dropout=0.0, tied=True, return_att=True))
    twice("tied row layer", lambda: m(msa))
    m2 = build(lambda: R.EncoderLayer(d_msa=DM, d_ff=4 * DM, n_heads=12, p_dropout=0.0, tied=False, performer=True))

    def col():
        x = msa.clone()
        m2.run(x, seq_axis=1)
        return x
    for _ in range(3):
        twice("performer column layer (FAVOR+ softmax features, 128-row sequences)", col)
    att = torch.rand(1, L2, L2, 12, generator=torch.Generator().manual_seed(2)).softmax(2).to(DEV)
    m3 = build(lambda: R.PairUpdateWithMsa(d_msa=DM, d_proj=32, d_pair=DP, n_heads=12, p_dropout=0.0))
    twice("pair update with msa", lambda: m3(msa, pair, att))
    m5 = build(lambda: R.PairUpdateWithAxialAttentionLayer(DP, 4 * DP, 8, 0.0, {}))
    twice("pair axial layer", lambda: m5(pair))
    m6 = build(lambda: R.MsaUpdateWithPair(DM, DP, 4, n_encoder_layers=1, p_dropout=0.0))
    twice("msa update with pair", lambda: m6(msa, pair))
    m9 = build(lambda: R.PredictionHead(DP, 4, 0.0))
    twice("prediction head", lambda: m9(pair))


@pytest.mark.parametrize("gen,Ls", [(True, 64), (True, 128), (True, 256), (False, 64), (False, 128), (False, 256)])
def test_fused_favor_run_to_run(gen, Ls):
    """The fused FAVOR+ kernel, every (feature map, sequence length) variant, 1024 x heads items: six runs bitwise equal."""
    from rosettafold_pytorch_amd import ops
    H, D, Lo = (12, 384, 1024) if Ls == 128 else (8, 288, 1024)
    torch.manual_seed(0)
    m = R.PerformerSelfAttention(dim=D, heads=H, generalized_attention=gen).to(DEV)
    inner, W3 = 64 * H, 3 * 64 * H
    qkv = torch.randn(Lo * Ls, W3, device=DEV).bfloat16()
    pc = m.proj_scaled(log2e=not gen)

    def f():
        o = torch.empty(Lo * Ls, inner, device=DEV, dtype=torch.bfloat16)
        ops.favor_attention(qkv, pc, o, (Lo * Ls * W3, Ls * W3, W3, 64), (Lo * Ls * inner, Ls * inner, inner), 0, inner,
                            2 * inner, 1, Lo, H, Ls, 64, 266, not gen, 1e-3 if gen else 1e-4)
        return o
    outs = [f() for _ in range(6)]
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0], o) for o in outs[1:])


# ---- round 4: regression tests for the round-3 advisor findings -----------------------------------------------------------------------
@pytest.mark.parametrize("dt,tol", [(torch.bfloat16, 2e-2), (torch.float16, 4e-3)], ids=["bf16", "fp16"])
def test_tied_row_layer_d_msa_288(dt, tol):
    """d_msa = 288 (9 heads of 32): the q|k|v projection has N = 864, which the register-resident-weights kernel does not take, so
    the position weights cannot ride in its epilogue (`rs`): the layer must fall back to applying them in the logits kernel
    instead of raising RF_EINVAL (round-3 advisor finding, model.py `fold`)."""
    from rosettafold_pytorch_amd import ops
    assert not ops.gemm_takes_row_scale(128 * 256, 3 * 288, 288) and ops.gemm_takes_row_scale(128 * 256, 3 * 384, 384)
    torch.manual_seed(21)
    m = R.EncoderLayer(d_msa=288, d_ff=4 * 288, n_heads=9, p_dropout=0.0, tied=True, return_att=True).to(DEV)
    x = rn(1, 128, 256, 288)
    with torch.no_grad():
        ro, ra = O.encoder_layer_tied(state(m), "m", x, 9)
    R.set_compute_dtype(dt)
    try:
        out, att = m(x.to(DEV))
    finally:
        R.set_compute_dtype(torch.bfloat16)
    assert rel(out, ro) < tol and rel(att, ra) < 2 * tol, (rel(out, ro), rel(att, ra))


def test_performer_gemm_chain_fp16_range_L1024():
    """fp16 operands (range 65504): the UNFUSED Performer chain (non-fused shapes, the sequence-sharded 'contexts' mode) stores the
    contexts k'^T v and the k' sums over the whole sequence in the 16-bit type; with large-magnitude keys / values at L = 1024 they
    leave fp16's range unless they are scaled by 2^-ceil(log2 L) as the fused kernel does (round-3 advisor finding)."""
    torch.manual_seed(22)
    m = R.PerformerSelfAttention(dim=288, heads=8, generalized_attention=True).to(DEV)
    with torch.no_grad():
        m.to_k.weight.mul_(6.0)
        m.to_v.weight.mul_(24.0)
    x = 3.0 * rn(2, 1024, 288)
    with torch.no_grad():
        ref = O.performer_self_attention(state(m), "m", x, 8, True)
    R.set_compute_dtype(torch.float16)
    old = R.RT.fused_favor
    try:
        R.RT.fused_favor = False      # the GEMM chain
        got = m(x.to(DEV))
    finally:
        R.RT.fused_favor = old
        R.set_compute_dtype(torch.bfloat16)
    assert torch.isfinite(got).all()
    assert rel(got, ref) < 1e-2, rel(got, ref)
