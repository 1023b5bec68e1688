#!/usr/bin/env python3
"""Golden fixture for the edge_mask argument of GraphTransformerBlock (build container only; needs /root/reference):

  * graph_transformer_block_masked.npz -- the reference's GraphTransformerBlock(8, 8, 8, 4, 0.0) at B=2, L=13 under a seeded
    Bernoulli(0.4) float32 mask [B, L, L] (1 = the edge exists, rf.py:635) in which row (0, 3) is empty, row (1, 0) is full and
    row (1, 5) keeps column 7 only: `in:node`, `in:edge`, `in:edge_mask`, `w:*`, `out:y`.

The empty row is the case worth pinning: the reference adds (1 - mask) * -1e9 to the scaled logits in float32, where the spacing
at 1e9 is 64, so a row without an edge comes out as the uniform 1/L whenever its scaled logits lie in (-32, 32).  The tool prints
the largest |scaled logit| of the case, the distance of the reference from a float64 restatement of that rule and the distance of
the masked output from the unmasked one.  Nothing of the reference is copied: it is imported at run time, with the inert
stand-ins of tools/make_goldens.py.

    python tools/make_goldens_edge_mask.py
"""
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as MG  # noqa: E402


def restate(P, node, edge, mask, H):
    """float64: softmax over a row's edges only; a row with no edge: uniform over all columns."""
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
        on = (mask == 1)[:, None]                                    # [B, 1, L, L]
        empty = ~on.any(-1, keepdim=True)
        logit = torch.where(empty, torch.zeros_like(logit), logit.masked_fill(~on, float("-inf")))
    att = logit.softmax(-1)
    upd = torch.einsum("bhij,bjhd->bihd", att, v) + torch.einsum("bhij,bijhd->bihd", att, e)
    x = lin(node, "attn.node_update") + upd.reshape(B, L, H * d)
    x = torch.nn.functional.layer_norm(x, (H * d,), P["ln.weight"], P["ln.bias"], 1e-5)
    return torch.nn.functional.elu(lin(x, "to_out.0")) + node, logit


def main():
    os.makedirs(MG.OUT, exist_ok=True)
    os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
    sys.dont_write_bytecode = True
    os.chdir(tempfile.mkdtemp(prefix="rf_golden_edge_mask_"))
    MG.install_standins()
    sys.path.insert(0, MG.REF)
    import rosettafold_pytorch.rosettafold_pytorch as rf

    torch.set_grad_enabled(False)
    g = torch.Generator().manual_seed(11)
    B, L, dn, de, H = 2, 13, 8, 8, 4
    node, edge = torch.randn(B, L, dn, generator=g), torch.randn(B, L, L, de, generator=g)
    mask = (torch.rand(B, L, L, generator=g) < 0.4).float()
    mask[0, 3] = 0.0
    mask[1, 0] = 1.0
    mask[1, 5] = 0.0
    mask[1, 5, 7] = 1.0
    torch.manual_seed(9)
    m = rf.GraphTransformerBlock(dn, dn, de, H, 0.0).eval()
    y = m(node, edge, mask.clone())
    MG.save("graph_transformer_block_masked", m, {"node": node, "edge": edge, "edge_mask": mask}, {"y": y}, {"n_heads": H})
    P = dict(m.state_dict())
    r, _ = restate(P, node, edge, mask, H)
    r0, logit = restate(P, node, edge, None, H)
    print(f"largest |scaled logit| {logit.abs().max().item():.3f} (the empty-row rule needs < 32)")
    print(f"reference - float64 restatement: max abs {(y.double() - r).abs().max().item():.2e}, "
          f"empty row (0, 3) {(y.double() - r)[0, 3].abs().max().item():.2e}")
    print(f"masked - unmasked restatement: max abs {(r - r0).abs().max().item():.3f}")


if __name__ == "__main__":
    main()
