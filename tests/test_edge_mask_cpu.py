"""CPU-side checks of the edge_mask route of GraphTransformer: the entry point is declared, bound and exported by both builds,
the dispatcher op exists with a fake implementation and stays out of custom_ops.OPS, and the masking rule itself -- a row
attends to its edges only, a row with no edge uniformly to every column -- reproduces the reference's own output
(tests/golden/graph_transformer_block_masked.npz, tools/make_goldens_edge_mask.py) when restated in float64.  No kernel is
launched."""
import os
import re

import numpy as np
import torch

import rosettafold_pytorch_amd as R  # noqa: F401
from rosettafold_pytorch_amd import _lib, custom_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "rfmi.h")) as fh:
        header = fh.read()
    assert re.search(r"\bint\s+rf_graph_attention_masked\s*\(", header)
    assert "rf_graph_attention_masked" in _lib.PROTOTYPES
    for handle in _lib.LIBS.values():
        assert callable(getattr(handle, "rf_graph_attention_masked"))
    assert _lib.lib.rf_version() >= 10


def test_custom_op_has_a_fake_implementation():
    op = torch.ops.rfmi.graph_transformer_masked
    B, L, H, d = 2, 7, 4, 8
    q = torch.empty(B, L, H, d, device="meta", dtype=torch.bfloat16)
    e = torch.empty(B, L, L, H * d, device="meta", dtype=torch.bfloat16)
    mask = torch.empty(B, L, L, device="meta", dtype=torch.uint8)
    y = op(q, q, q, e, mask, 0.35)
    assert y.device.type == "meta" and tuple(y.shape) == (B, L, H * d) and y.dtype == torch.float32


def test_ops_tuple_is_unchanged():
    assert len(custom_ops.OPS) == 18
    assert "graph_transformer_masked" not in custom_ops.OPS
    assert "graph_transformer_masked" in custom_ops.MASKED_OPS


def restate(P, node, edge, mask, H):
    """GraphTransformerBlock in float64 under the masking rule: softmax over a row's edges only (mask == 1), masked columns
    exactly 0; a row with no edge: the uniform 1/L over all columns.  mask None: the dense graph."""
    P = {k: v.double() for k, v in P.items()}
    node, edge = node.double(), edge.double()
    B, L, _ = node.shape

    def lin(x, name, bias=True):
        y = x @ P[name + ".weight"].T
        return y + P[name + ".bias"] if bias else y

    q, k, v = (lin(node, "attn.node_to_" + c).view(B, L, H, -1) for c in "qkv")
    d = q.shape[-1]
    e = lin(edge, "attn.edge_emb", bias=False).view(B, L, L, H, d)
    logit = (torch.einsum("bihd,bjhd->bhij", q, k) + torch.einsum("bihd,bijhd->bhij", q, e)) * d ** -0.5
    if mask is not None:
        on = (mask == 1)[:, None]
        empty = ~on.any(-1, keepdim=True)
        logit = torch.where(empty, torch.zeros_like(logit), logit.masked_fill(~on, float("-inf")))
    att = logit.softmax(-1)
    upd = torch.einsum("bhij,bjhd->bihd", att, v) + torch.einsum("bhij,bijhd->bihd", att, e)
    x = lin(node, "attn.node_update") + upd.reshape(B, L, H * d)
    x = torch.nn.functional.layer_norm(x, (H * d,), P["ln.weight"], P["ln.bias"], 1e-5)
    return torch.nn.functional.elu(lin(x, "to_out.0")) + node


def test_masking_rule_reproduces_the_reference(golden_dir):
    z = np.load(os.path.join(golden_dir, "graph_transformer_block_masked.npz"), allow_pickle=False)
    P = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}
    node, edge, mask = (torch.from_numpy(z["in:" + k]) for k in ("node", "edge", "edge_mask"))
    want = torch.from_numpy(z["out:y"])
    assert mask.dtype == torch.float32 and tuple(mask.shape) == (2, 13, 13)
    deg = (mask == 1).sum(-1)
    assert deg[0, 3] == 0 and deg[1, 0] == 13 and deg[1, 5] == 1 and mask[1, 5, 7] == 1   # the rows the fixture is about
    got = restate(P, node, edge, mask, int(z["x:n_heads"]))
    torch.testing.assert_close(got.float(), want, rtol=1e-4, atol=2e-5)
    dense = restate(P, node, edge, None, int(z["x:n_heads"]))
    assert (got - dense).abs().max().item() > 0.1   # a dropped mask cannot pass
    assert (got - dense)[0, 3].abs().max().item() > 1e-3   # nor can an empty row that kept its dense softmax
