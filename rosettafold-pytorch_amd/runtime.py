"""Process-wide runtime state of the HIP path (compute dtype, switches, the training-mode dropout stream) and the few helpers
that both the forward (model.py) and the backward machinery (backward.py) need.  model.py re-exports every name here."""
import torch

from . import ops
from .ops import F32


class _Runtime:
    dtype = torch.bfloat16
    f32_precision = "highest"  # set_float32_matmul_precision: "high" = split-bf16 GEMMs in the float32 mode
    # training-mode dropout: masks are Philox4x32-10(train_seed, counter); every dropout call of a forward
    # takes the next ceil(n / 4) counters, so manual_seed(s) in front of a forward reproduces it bit for bit (csrc/ops.hip)
    train_seed = 0
    train_offset = 0
    cache_epoch = 0  # bumped whenever kernel-ready weight copies are dropped (graph.GraphedForward re-records on a change)
    # structure-track node input (LayerNorm(msa) -> position-weighted sum, rf.py:789-798) in fp32 also in the 16-bit modes:
    # the SE(3) stack is discontinuous (GNormBias, kNN, distance bins), so its inputs are not the place to round
    # (tools/depth_parity.py --struct-lowp measures the difference)
    struct_inputs_fp32 = True
    # PredictionHead: remove the per-(sample, channel) mean over the picture from the projected pair tensor before it is rounded
    # to the 16-bit operand type (PredictionHead.run; RF_HEAD_CENTER=0 restores the plain cast)
    head_center = bool(int(__import__("os").environ.get("RF_HEAD_CENTER", "1")))
    # Operand conditioning of the 16-bit modes (csrc/condition.hip; exact algebra): PairUpdateWithMsa's tiled 1-D features and its
    # first convolution see operands with the per-sample constant removed.  RF_CONDITION=0: the plain form (ablation / probes).
    condition = bool(int(__import__("os").environ.get("RF_CONDITION", "1")))
    condition_values = bool(int(__import__("os").environ.get("RF_CONDITION_V", "1")))   # the attention layers' value path (value_conditioning)
    # SE(3) radial MLPs: last Linear inside the message kernel (csrc/se3.hip: rf_se3_radial_message); RF_SE3_UNFUSED=1 writes the
    # radial outputs with a K = 32 GEMM and reads them back (round-3 path, kept for A/B timing and as the form for unusual shapes)
    se3_fused_radial = not bool(int(__import__("os").environ.get("RF_SE3_UNFUSED", "0")))
    fused_favor = True  # use the fused FAVOR+ kernel where ops.favor_fused_applies holds (16-bit modes, dim_head 64, any length from its floor up)
    fused_outer_ln = not bool(int(__import__("os").environ.get("RF_NO_FUSED_OUTER_LN", "0")))  # LayerNorm(1024) in the outer-product GEMM epilogue
    fused_tied = not bool(int(__import__("os").environ.get("RF_NO_FUSED_TIED", "0")))  # tied-attention logits + softmax in one launch
    fused_outer = not bool(int(__import__("os").environ.get("RF_NO_FUSED_OUTER", "0")))  # outer product -> LN -> Linear in one kernel
    # OuterProductMean backward (model.py): the pair picture is walked in slabs of rows whose three P^2-wide tensors (outer
    # products / LN(o), dz / do, do transposed) together stay under this many bytes; RF_OUTER_BWD_SLAB_MB sets it.  The
    # LayerNorm step of a slab is one launch of rf_layernorm_bwd_fused; RF_NO_FUSED_OUTER_BWD=1 runs it as the chain of the
    # older engines (rf_layernorm, two casts, rf_layernorm_bwd) for A/B timing (tools/outer_backward_bench.py).
    outer_bwd_slab_bytes = int(float(__import__("os").environ.get("RF_OUTER_BWD_SLAB_MB", "6")) * (1 << 20))
    outer_bwd_fused = not bool(int(__import__("os").environ.get("RF_NO_FUSED_OUTER_BWD", "0")))
    tied_v2 = not bool(int(__import__("os").environ.get("RF_TIED_V1", "0")))  # head-major q|k|v + collapsed weights + A.V kernel
    tied_fold_w = not bool(int(__import__("os").environ.get("RF_TIED_NO_FOLD", "0")))  # position weights folded into q by the projection's epilogue
    # long rows off 512 / 768 / 1024 (any 257 <= L <= 1024) on the tail instantiations of the contraction-split logits kernel;
    # RF_NO_TIED_LONG_RAGGED=1 restores the general route at these lengths, for A/B timing (tools/tied_long_ragged_bench.py)
    tied_long_ragged = not bool(int(__import__("os").environ.get("RF_NO_TIED_LONG_RAGGED", "0")))
    # pair-track row blocks (shard.forward_row_sharded): how the attention direction that crosses the blocks is computed --
    # "transpose" (two transposing exchanges, fused kernel) or "contexts" (all-reduce of the Performer contexts, GEMM chain)
    rowshard_attention = __import__("os").environ.get("RF_ROWSHARD_ATTENTION", "transpose")


RT = _Runtime()


def T():
    return RT.dtype


def manual_seed(seed):
    """Seed of the training-mode dropout masks (model.train(); the inference forward draws nothing).  Like torch.manual_seed:
    the same seed in front of the same forward gives the same masks; consecutive forwards continue the counter stream."""
    RT.train_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    RT.train_offset = 0


def dropout_(t, p):
    """In-place nn.Dropout(p) of a training-mode forward on a contiguous fp32 / 16-bit tensor (rf_dropout); identity for p <= 0."""
    if p is None or p <= 0.0 or t.numel() == 0:
        return t
    if p >= 1.0:
        return ops.fill(t, 0.0)
    if not t.is_contiguous():
        raise ValueError("dropout_: contiguous tensors only")
    off = RT.train_offset
    RT.train_offset += (t.numel() + 3) // 4
    return ops.dropout(t, p, RT.train_seed, off)


def _f(p):
    return None if p is None else p.detach()


def fresh_f32(x):
    """A new contiguous fp32 copy of x (the public forwards never mutate their inputs)."""
    y = torch.empty(x.shape, device=x.device, dtype=F32)
    return ops.axpby(x.detach().contiguous(), 1.0, None, 0.0, y)
