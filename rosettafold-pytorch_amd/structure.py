"""Structure track (SE(3)-Transformer over the kNN residue graph), the three-track blocks and the
top-level RoseTTAFold module.  Mirrors rf.py:752-1289, se3_modules.py:83-171 and the used classes of
equivariant_attention/modules.py (parameter names included) over the fp32 kernels of csrc/se3.hip."""
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .ops import F32
from .model import (RFModule, RecordingModule, Residual, FeedForward, PositionWiseWeightFactor, MsaEmbedding, PairEmbedding,
                    MsaUpdateUsingSelfAttention, PairUpdateWithMsa, PairUpdateWithAxialAttention, MsaUpdateWithPair,
                    InitialCoordGenerationWithMsaAndPair, PredictionHead, LayerNorm, Linear, _node_input, _f, ln, T, pad8,
                    CA_IDX, fresh_f32, check_index_range, RT)
from .backward import (_recording, _RecordedFn, _check_backward_call, _copy, _grad_scale, _scaled_copy, _unscale,
                       _pre_norm_residual_bwd)


# ================================================================================================
# SE(3)-Transformer parameter containers (names as in ea/modules.py) + device forward
# ================================================================================================
class BN(nn.Module):
    """ea/modules.py:545-558 (a LayerNorm)."""

    def __init__(self, m):
        super().__init__()
        self.bn = LayerNorm(m)


class RadialFunc(nn.Module):
    """ea/modules.py:246-284."""

    def __init__(self, num_freq, in_dim, out_dim, edge_dim=0):
        super().__init__()
        self.num_freq, self.in_dim, self.out_dim, self.edge_dim, self.mid_dim = num_freq, in_dim, out_dim, edge_dim, 32
        self.net = nn.Sequential(Linear(edge_dim + 1, 32), BN(32), nn.ReLU(), Linear(32, 32), BN(32), nn.ReLU(),
                                 Linear(32, num_freq * in_dim * out_dim))
        nn.init.kaiming_uniform_(self.net[0].weight)
        nn.init.kaiming_uniform_(self.net[3].weight)
        nn.init.kaiming_uniform_(self.net[6].weight)


class PairwiseConv(nn.Module):
    """ea/modules.py:287-325."""

    def __init__(self, degree_in, nc_in, degree_out, nc_out, edge_dim=0):
        super().__init__()
        self.degree_in, self.degree_out, self.nc_in, self.nc_out = degree_in, degree_out, nc_in, nc_out
        self.num_freq = 2 * min(degree_in, degree_out) + 1
        self.rp = RadialFunc(self.num_freq, nc_in, nc_out, edge_dim)


class GConvSE3Partial(nn.Module):
    """ea/modules.py:561-680 (x_ij=None)."""

    def __init__(self, f_in, f_out, edge_dim=0):
        super().__init__()
        self.f_in, self.f_out = dict(f_in), dict(f_out)
        self.kernel_unary = nn.ModuleDict()
        for di, mi in f_in.items():
            for do, mo in f_out.items():
                self.kernel_unary[f"({di},{do})"] = PairwiseConv(di, mi, do, mo, edge_dim=edge_dim)


class _FiberModule(RecordingModule):
    """A node layer of the SE(3)-Transformer on the reference's fiber dicts h = {degree: fp32 [V, m, 2 degree + 1]}, degrees 0 and
    1, with the opt-in backward of backward.py: `run(h, tape=None)` is the kernel sequence, `_backward(tape, g)` with
    g = {output degree: contiguous fp32 gradient} returns ({input degree: gradient}, {param: grad}).  forward(h) returns the dict
    run returns; with enable_backward() and grad mode on it records, one tensor input per degree (an absent degree is None) and
    one output per output degree.  The structure track is fp32 in every compute mode: nothing here reads the compute dtype, the
    gradients carry no fp16 scale (_rf_scales_own_grads) and the same bits come out under every set_compute_dtype.  Tapes hold
    inputs only.  GSE3Res, SE3Transformer, CoordUpdateWithMsaAndPair and RoseTTAFold.forward call run() without a tape: they
    never record here."""
    _rf_n_inputs = 2   # the degree-0 and the degree-1 features
    _rf_scales_own_grads = True

    def _out_degrees(self, h):
        return sorted(h)

    def _record(self, x0, x1, tape):
        h = {d: x.float().contiguous() for d, x in ((0, x0), (1, x1)) if x is not None}
        out = self.run(h, tape=tape)
        return out if tape is None else tuple(out[d] for d in self._out_degrees(h))

    def _backward_from_autograd(self, tape, gs, s, want):
        g = {d: _scaled_copy(gi, 1.0) for d, gi in zip(self._out_degrees(tape["h"]), gs)}
        dh, grads = self._backward(tape, g)
        return (dh.get(0), dh.get(1)), grads

    def forward(self, h):
        if _recording(self):
            return dict(zip(self._out_degrees(h), _RecordedFn.apply(self, h.get(0), h.get(1), *self.parameters())))
        return self._record(h.get(0), h.get(1), None)


class G1x1SE3(_FiberModule):
    """ea/modules.py:328-361.  enable_backward(): the gradients of the transforms and of the input degrees of f_out (an input
    degree f_out does not name is not read and gets none)."""

    def __init__(self, f_in, f_out):
        super().__init__()
        self.f_in, self.f_out = dict(f_in), dict(f_out)
        self.transform = nn.ParameterDict()
        for do, mo in f_out.items():
            mi = f_in[do]
            self.transform[str(do)] = nn.Parameter(torch.randn(mo, mi) / np.sqrt(mi))

    def _out_degrees(self, h):
        return sorted(self.f_out)

    def run(self, h, tape=None):
        out = {}
        for d in self.f_out:
            x = h[d]
            V, mi, nc = x.shape
            W = self.transform[str(d)].detach()
            mo = W.shape[0]
            y = torch.empty(V, mo, nc, device=x.device, dtype=F32)
            ops.gemm(x, W, y, V * nc, mo, mi, kc=1, a_row=(nc, mi * nc, 1), a_ko=nc, b_row=(0, 0, mi), b_ko=1,
                     c_row=(nc, mo * nc, 1), c_col=(1, nc), exact=True)
            out[d] = y
        if tape is not None:
            tape["h"] = {d: h[d] for d in self.f_out}
        return out

    def _backward(self, tape, g):
        """Both contractions on the exact fp32 rf_gemm, whose strides express them at any channel count:
            dx[v,i,c] = sum_o W[o,i] g[v,o,c]         the forward's call on g and W^T
            dW[o,i]   = sum_{v,c} g[v,o,c] x[v,i,c]    K = (v, c) in chunks of 2 d + 1, a node apart"""
        dh, grads = {}, {}
        for d, x in tape["h"].items():
            V, mi, nc = x.shape
            W = self.transform[str(d)]
            mo = W.shape[0]
            wt = ops.copy(W.detach().t(), torch.empty(mi, mo, device=x.device, dtype=F32))
            dx = torch.empty_like(x)
            ops.gemm(g[d], wt, dx, V * nc, mi, mo, kc=1, a_row=(nc, mo * nc, 1), a_ko=nc, b_row=(0, 0, mo), b_ko=1,
                     c_row=(nc, mi * nc, 1), c_col=(1, nc), exact=True)
            dw = torch.empty(mo, mi, device=x.device, dtype=F32)
            ops.gemm(g[d], x, dw, mo, mi, V * nc, kc=nc, a_row=(0, 0, nc), a_ko=mo * nc, b_row=(0, 0, nc), b_ko=mi * nc, exact=True)
            dh[d], grads[W] = dx, dw
        return dh, grads


class GNormBias(_FiberModule):
    """ea/modules.py:364-406.  enable_backward(): the gradients of the biases and of the input (rf_se3_norm_bias_bwd)."""

    def __init__(self, fiber):
        super().__init__()
        self.bias = nn.ParameterDict({str(d): nn.Parameter(torch.randn(m).view(1, m)) for d, m in fiber.items()})

    def run(self, h, tape=None):
        if tape is not None:
            tape["h"] = dict(h)
        return {d: ops.se3_norm_bias(v, self.bias[str(d)].detach().reshape(-1), d) for d, v in h.items()}

    def _backward(self, tape, g):
        dh, grads = {}, {}
        for d, v in tape["h"].items():
            b = self.bias[str(d)]
            dh[d], db = ops.se3_norm_bias_bwd(v, b.detach().reshape(-1), g[d], d)
            grads[b] = db.view(b.shape)
        return dh, grads


class GAttentiveSelfInt(_FiberModule):
    """ea/modules.py:409-473.  enable_backward(): the gradients of each degree's LayerNorm and Linear and of the input."""

    def __init__(self, f_in, f_out):
        super().__init__()
        self.f_in, self.f_out = dict(f_in), dict(f_out)
        self.transform = nn.ModuleDict()
        for d, mi in f_in.items():
            mo = f_out[d]
            lin = Linear(mi * mi, mi * mo, bias=True)
            nn.init.kaiming_uniform_(lin.weight)
            self.transform[str(d)] = nn.Sequential(LayerNorm(mi * mi), nn.LeakyReLU(), lin)

    def _front(self, d, v):
        """the Gram matrix, its LayerNorm + LeakyReLU and the attention logits of degree d"""
        net = self.transform[str(d)]
        s = ops.se3_gram(v, d)
        t = ops.layernorm(s, _f(net[0].weight), _f(net[0].bias), eps=net[0].eps, out_dtype=F32, act=L.ACT_LEAKY)
        a = ops.linear(t, net[2].weight.detach(), _f(net[2].bias), out_dtype=F32, exact=True)
        return s, t, a

    def run(self, h, tape=None):
        if tape is not None:
            tape["h"] = dict(h)
        return {d: ops.se3_attn_apply(self._front(d, v)[2], v, self.f_out[d], d) for d, v in h.items()}

    def _backward(self, tape, g):
        """Per degree, with s, t, a rebuilt from v by the forward's own launches:
            d a, d v  = rf_se3_attn_apply_bwd(a, v, g)                    the apply path's share of d v
            dW, db    = d a^T t, sum d a                                  rf_conv_wgrad in fp32 (exact, any channel count)
            d t       = d a W                                             rf_gemm, exact fp32
            d s, dgamma, dbeta = rf_layernorm_act_bwd(s, d t)             LayerNorm + LeakyReLU over m_in^2 values
            d v      += rf_se3_gram_bwd(v, d s)                           into the same tensor: v is read twice"""
        dh, grads = {}, {}
        for d, v in tape["h"].items():
            net = self.transform[str(d)]
            lnm, lin = net[0], net[2]
            s, t, a = self._front(d, v)
            da, dv = ops.se3_attn_apply_bwd(a, v, g[d], self.f_out[d], d)
            grads[lin.weight], grads[lin.bias] = ops.conv_wgrad(da, t, 1, bias=True)
            wt = ops.copy(lin.weight.detach().t(), torch.empty(lin.in_features, lin.out_features, device=v.device, dtype=F32))
            dt = ops.linear(da, wt, None, out_dtype=F32, exact=True)
            ds, grads[lnm.weight], grads[lnm.bias] = ops.layernorm_act_bwd(s, dt, _f(lnm.weight), _f(lnm.bias), eps=lnm.eps,
                                                                          act=L.ACT_LEAKY)
            dh[d] = ops.se3_gram_bwd(v, ds, d, dv=dv)
        return dh, grads


class GMABSE3(RecordingModule):
    """ea/modules.py:683-774 (no parameters) with the skip concatenation behind it (GCat, ea/modules.py:903-928).
    run(v, k, q, g, skip=None): v, k per-edge and q per-node fiber dicts of degrees 0 and 1, g the graph dict of build_graph (its
    eid, V and L are read), skip a fiber dict of node features or None.  Returns {degree: [V, mv (+ skip channels), 2 degree + 1]}:
    the attention in the leading channels, the skip features behind them.  enable_backward(): with grad mode on,
    forward(v, k, q, g, skip=None) records and the gradient reaches v, k, q and skip (rf_se3_attention_bwd on the leading channels
    of the output's gradient; the trailing channels are the skip's gradient, bit for bit); the graph takes none.  Rows of the
    per-edge gradients at or above the edge count are not written.  fp32 in every compute mode, like the node layers."""
    _rf_n_inputs = 9   # v0, v1, k0, k1, q0, q1, skip0, skip1 (either may be None), the graph (no gradient)
    _rf_scales_own_grads = True

    def __init__(self, f_value, f_key, n_heads):
        super().__init__()
        self.f_value, self.f_key, self.n_heads = dict(f_value), dict(f_key), n_heads

    def run(self, v, k, q, g, skip=None, tape=None):
        skip = skip or {}
        fk, fv = self.f_key, self.f_value
        if tape is not None:
            tape.update(v=dict(v), k=dict(k), q=dict(q), g=g, skip={d: x.shape for d, x in skip.items()})
        z0, z1 = ops.se3_attention(k[0], k[1], q[0], q[1], v[0], v[1], g["eid"], self.n_heads, fk[0], fk[1], fv[0], fv[1],
                                   g["V"], g["L"], skip0=skip.get(0), skip1=skip.get(1))
        return {0: z0, 1: z1}

    def _backward(self, tape, gz):
        """gz: {degree: contiguous fp32 gradient of the concatenated output}.  Returns ({"v", "k", "q", "skip": fiber dicts}, {})."""
        v, k, q, g = tape["v"], tape["k"], tape["q"], tape["g"]
        fk, fv = self.f_key, self.f_value
        dk0, dk1, dq0, dq1, dv0, dv1 = ops.se3_attention_bwd(k[0], k[1], q[0], q[1], v[0], v[1], g["eid"], gz[0], gz[1],
                                                             self.n_heads, fk[0], fk[1], fv[0], fv[1], g["V"], g["L"])
        dskip = {d: ops.copy(gz[d][:, fv[d]:], torch.empty(shape, device=gz[d].device, dtype=F32))
                 for d, shape in tape["skip"].items()}
        return {"v": {0: dv0, 1: dv1}, "k": {0: dk0, 1: dk1}, "q": {0: dq0, 1: dq1}, "skip": dskip}, {}

    def _record(self, v0, v1, k0, k1, q0, q1, s0, s1, g, tape):
        c = lambda x: x.float().contiguous()  # noqa: E731
        out = self.run({0: c(v0), 1: c(v1)}, {0: c(k0), 1: c(k1)}, {0: c(q0), 1: c(q1)}, g,
                       {d: c(x) for d, x in ((0, s0), (1, s1)) if x is not None}, tape=tape)
        return out if tape is None else (out[0], out[1])

    def _backward_from_autograd(self, tape, gs, s, want):
        d, _ = self._backward(tape, {0: _scaled_copy(gs[0], 1.0), 1: _scaled_copy(gs[1], 1.0)})
        return (d["v"][0], d["v"][1], d["k"][0], d["k"][1], d["q"][0], d["q"][1], d["skip"].get(0), d["skip"].get(1), None), {}

    def forward(self, v, k, q, g, skip=None):
        if g["L"] > 1024:
            raise ValueError(f"GMABSE3: the graph attention covers chains of up to 1024 residues, got {g['L']}")
        skip = skip or {}
        args = (v[0], v[1], k[0], k[1], q[0], q[1], skip.get(0), skip.get(1), g)
        if _recording(self):
            return dict(zip((0, 1), _RecordedFn.apply(self, *args)))
        return self._record(*args, None)


def _pack_radial_net(rp):
    """[W1^T: ki x 32][b1][ln1 gamma][ln1 beta][W2^T: 32 x 32][b2][ln2 gamma][ln2 beta][W3: rows x 32][b3: rows] fp32."""
    n = rp.net
    parts = [n[0].weight.t(), n[0].bias, n[1].bn.weight, n[1].bn.bias, n[3].weight.t(), n[3].bias, n[4].bn.weight, n[4].bn.bias,
             n[6].weight, n[6].bias]
    return torch.cat([t.detach().float().contiguous().reshape(-1) for t in parts]).contiguous()


class GSE3Res(nn.Module):
    """ea/modules.py:777-857 with skip='cat'."""

    def __init__(self, f_in, f_out, edge_dim=0, div=4, n_heads=1, selfint="1x1"):
        super().__init__()
        self.f_in, self.f_out, self.n_heads, self.edge_dim = dict(f_in), dict(f_out), n_heads, edge_dim
        self.f_mid_out = {d: int(m // div) for d, m in f_out.items()}
        self.f_mid_in = {d: m for d, m in self.f_mid_out.items() if d in f_in}
        self.GMAB = nn.ModuleDict()
        self.GMAB["v"] = GConvSE3Partial(f_in, self.f_mid_out, edge_dim=edge_dim)
        self.GMAB["k"] = GConvSE3Partial(f_in, self.f_mid_in, edge_dim=edge_dim)
        self.GMAB["q"] = G1x1SE3(f_in, self.f_mid_in)
        self.GMAB["attn"] = GMABSE3(self.f_mid_out, self.f_mid_in, n_heads=n_heads)
        f_cat = {d: m + f_in.get(d, 0) for d, m in self.f_mid_out.items()}  # GCat ea/modules.py:903-928
        self.f_cat = f_cat
        self.project = GAttentiveSelfInt(f_cat, f_out) if selfint == "att" else G1x1SE3(f_cat, f_out)
        object.__setattr__(self, "_rfc", None)

    def _nets(self):
        """[(which, di, do, PairwiseConv)] in a fixed order; radial first/second layers are batched over them."""
        nets = []
        for which in ("v", "k"):
            conv = self.GMAB[which]
            for di in conv.f_in:
                for do in conv.f_out:
                    nets.append((which, di, do, conv.kernel_unary[f"({di},{do})"]))
        return nets

    def _packed(self):
        if not self._rfc:  # (None, or emptied by invalidate_weight_caches)
            nets = self._nets()
            with torch.no_grad():
                pk = {
                    "w1": torch.cat([n[3].rp.net[0].weight for n in nets], 0).float().contiguous(),
                    "b1": torch.cat([n[3].rp.net[0].bias for n in nets], 0).float().contiguous(),
                    "g1": torch.cat([n[3].rp.net[1].bn.weight for n in nets], 0).float().contiguous(),
                    "e1": torch.cat([n[3].rp.net[1].bn.bias for n in nets], 0).float().contiguous(),
                    "g2": torch.cat([n[3].rp.net[4].bn.weight for n in nets], 0).float().contiguous(),
                    "e2": torch.cat([n[3].rp.net[4].bn.bias for n in nets], 0).float().contiguous(),
                    # one flat fp32 buffer per net in the order the fused kernel reads it (include/rfmi.h: rf_se3_radial_message)
                    "nets": {(which, di, do): _pack_radial_net(pc.rp) for which, di, do, pc in nets},
                }
            object.__setattr__(self, "_rfc", pk)
        return self._rfc

    def _apply(self, fn, *a, **k):
        object.__setattr__(self, "_rfc", None)
        RT.cache_epoch += 1
        return super()._apply(fn, *a, **k)

    def _load_from_state_dict(self, *a, **k):
        object.__setattr__(self, "_rfc", None)  # packed radial weights are rebuilt from the loaded parameters
        RT.cache_epoch += 1
        return super()._load_from_state_dict(*a, **k)

    def run(self, h, g):
        """h: {0: [V,m0,1], 1: [V,m1,3]} fp32;  g: graph dict (src, dst, eid, count, basis, feat, cap, V, L)."""
        nets = self._nets()
        G = len(nets)
        pk = self._packed()
        cap, feat = g["cap"], g["feat"]
        eps = nets[0][3].rp.net[1].bn.eps
        h0 = h.get(0)
        h1f = h.get(1)
        mi0 = h0.shape[1] if h0 is not None else 0
        mi1 = h1f.shape[1] if h1f is not None else 0
        ki = feat.shape[1]
        slot = {(which, di, do): gi for gi, (which, di, do, _) in enumerate(nets)}
        last = {(which, di, do): pc.rp.net[6] for which, di, do, pc in nets}
        todo = [(which, do, mo) for which, fo in (("v", self.f_mid_out), ("k", self.f_mid_in)) for do, mo in fo.items()]
        fused = {(which, do): RT.se3_fused_radial and ops.se3_radial_message_supported(
            mo, do, mi0 if (which, 0, do) in last else 0, mi1 if (which, 1, do) in last else 0, ki) for which, do, mo in todo}
        h2 = None
        if not all(fused.values()):
            # radial MLPs as launches (shapes without a fused instance, or RF_SE3_UNFUSED=1): layer 1 for all G nets in one GEMM,
            # grouped LayerNorm + ReLU, per-net 32x32 layer, grouped LayerNorm + ReLU; the output layer follows per net below
            h1 = ops.linear(feat, pk["w1"], pk["b1"], out_dtype=F32, exact=True)  # [cap, G*32]
            h1 = ops.layernorm(h1, pk["g1"], pk["e1"], eps=eps, out_dtype=F32, rows=cap * G, D=32, groups=G, act=L.ACT_RELU)
            h2 = torch.empty_like(h1)
            for gi, n in enumerate(nets):
                lin = n[3].rp.net[3]
                ops.gemm(h1, lin.weight.detach(), h2, cap, 32, 32, a_off=gi * 32, a_row=(0, 0, G * 32), c_off=gi * 32,
                         c_row=(0, 0, G * 32), bias=_f(lin.bias), exact=True)
            h2 = ops.layernorm(h2, pk["g2"], pk["e2"], eps=eps, out_dtype=F32, rows=cap * G, D=32, groups=G, act=L.ACT_RELU)
        msg = {}
        for which, do, mo in todo:
            has0, has1 = (which, 0, do) in last, (which, 1, do) in last
            if fused[(which, do)]:
                # the whole radial MLP inside the message kernel: no hidden vectors, no [cap, mo*mi*nf] radial tensors in memory
                msg[(which, do)] = ops.se3_radial_message(
                    feat, ki, pk["nets"].get((which, 0, do)), pk["nets"].get((which, 1, do)), g["basis"],
                    h0 if has0 else None, h1f if has1 else None, g["src"], g["count"], mo, do,
                    mi0 if has0 else 0, mi1 if has1 else 0, eps, cap)
                continue
            R = {}
            for di in (0, 1):
                lin = last.get((which, di, do))
                if lin is None:
                    continue
                nout = lin.weight.shape[0]
                r = torch.empty(cap, nout, device=feat.device, dtype=F32)
                ops.gemm(h2, lin.weight.detach(), r, cap, nout, 32, a_off=slot[(which, di, do)] * 32, a_row=(0, 0, G * 32),
                         bias=_f(lin.bias), exact=True)
                R[di] = r
            msg[(which, do)] = ops.se3_message(R.get(0), R.get(1), g["basis"], h0, h1f, g["src"], g["count"], mo, do, mi0, mi1, cap)
        q = self.GMAB["q"].run(h)
        # skip connection 'cat' (GCat, ea/modules.py:903-928): the attention writes the leading channels of the
        # concatenated buffers, the node's input features are copied in behind them
        z = self.GMAB["attn"].run({0: msg[("v", 0)], 1: msg[("v", 1)]}, {0: msg[("k", 0)], 1: msg[("k", 1)]}, q, g, skip=h)
        return self.project.run(z)


class SE3Transformer(nn.Module):
    """se3_modules.py:83-171 as instantiated at rf.py:774-784."""

    def __init__(self, num_layers=2, num_channels=32, num_degrees=3, n_heads=4, div=4, si_m="1x1", si_e="att",
                 l0_in_features=32, l0_out_features=32, l1_in_features=3, l1_out_features=3, num_edge_features=32,
                 x_ij=None):
        super().__init__()
        if num_degrees != 2 or x_ij is not None or l1_out_features <= 0:
            raise NotImplementedError("only the configuration used by the forward path (rf.py:774-784) is built")
        f_in = {0: l0_in_features, 1: l1_in_features}
        f_mid = {d: num_channels for d in range(num_degrees)}
        f_out = {0: l0_out_features, 1: l1_out_features}
        blocks = []
        fin = f_in
        for _ in range(num_layers):
            blocks.append(GSE3Res(fin, f_mid, edge_dim=num_edge_features, div=div, n_heads=n_heads, selfint=si_m))
            blocks.append(GNormBias(f_mid))
            fin = f_mid
        blocks.append(GSE3Res(f_mid, f_out, edge_dim=num_edge_features, div=1, n_heads=min(1, 2), selfint=si_e))
        self.Gblock = nn.ModuleList(blocks)

    def run(self, g, type0, type1):
        h = {0: type0, 1: type1}
        for blk in self.Gblock:
            h = blk.run(h, g) if isinstance(blk, GSE3Res) else blk.run(h)
        return h


_PENDING_EDGE_COUNTS = []   # (count tensor [min(edges, cap), edges], capacity) of the graphs built since the last check


def check_edge_capacity(pending=None):
    """Raises if a kNN graph had more edges than its static capacity (rf_edges_from_mask drops the overflow and reports the
    true count in count[1]): the capacity bound k + 2*(kmin-1) per row holds for strictly increasing residue indices,
    which the public forward()s verify -- this is the backstop behind that argument.  One 8-byte read-back per graph,
    taken at the END of a public forward (the launches are already queued; no bubble in front of them).
    `pending`: explicit list (graph.GraphedForward keeps the captured graph's counts); default: everything recorded since
    the last check, which is cleared."""
    items = pending if pending is not None else list(_PENDING_EDGE_COUNTS)
    if pending is None:
        _PENDING_EDGE_COUNTS.clear()
    for count, cap in items:
        kept, total = count.tolist()
        if total > cap:
            raise L.RfmiError(f"kNN graph overflow: {total} edges for a capacity of {cap} (residue indices not strictly "
                              f"increasing?) -- {total - kept} edges were dropped, the result is not the reference's")


def build_graph(xyz, edge_emb, aa_idx, n_neighbors, kmin=9, monotonic=True):
    """rf.py:823-862 on the device: dense mask -> compacted edge list (+ dense edge-id map) -> per-edge geometry.
    The edge count stays on the device; every per-edge buffer has a static capacity: B*L*min(L, k+2*(kmin-1)) when
    aa_idx is strictly increasing inside each sample (at most 2*(kmin-1) sequence neighbours besides the k nearest),
    B*L*L otherwise.  The compaction kernel never writes past the capacity (rf_edges_from_mask)."""
    B, Lr = xyz.shape[:2]
    k = min(n_neighbors, Lr)
    per_row = min(Lr, k + 2 * (kmin - 1)) if monotonic else Lr
    cap = (B * Lr * per_row + 63) // 64 * 64
    mask = ops.knn_mask(xyz, aa_idx, k, kmin)
    src, dst, eid, count = ops.edges_from_mask(mask, cap)
    _PENDING_EDGE_COUNTS.append((count, cap))
    del _PENDING_EDGE_COUNTS[:-64]   # callers of the internal run() paths never check: keep the list bounded
    basis, feat = ops.se3_edge_geometry(xyz, edge_emb, src, dst, count, cap)
    return {"src": src, "dst": dst, "eid": eid, "count": count, "basis": basis, "feat": feat, "cap": cap,
            "V": B * Lr, "L": Lr, "mask": mask}


class CoordUpdateWithMsaAndPair(RFModule):
    """rf.py:752-862."""

    def __init__(self, d_msa, d_pair, d_node, d_edge, d_state, n_neighbors, p_dropout=0.1):
        super().__init__()
        self.n_neighbors = n_neighbors
        self.ln_msa = LayerNorm(d_msa)
        self.ln_pair = LayerNorm(d_pair)
        self.poswise_weight = PositionWiseWeightFactor(d_msa, 1, p_dropout)
        self.node_embed = nn.Sequential(Linear(d_msa + 21, d_node), nn.ELU(), LayerNorm(d_node))
        self.edge_embed = nn.Sequential(Linear(d_pair, d_edge), nn.ELU(), LayerNorm(d_edge))
        self.se3_transformer = SE3Transformer(num_layers=2, num_channels=16, n_heads=4, num_degrees=2,
                                              l0_in_features=d_node, l1_in_features=3, l0_out_features=d_state,
                                              l1_out_features=3, num_edge_features=d_edge)

    def run(self, xyz, msa, pair, aa_idx, seq_onehot, monotonic=True):
        B, Lr = xyz.shape[:2]
        # the structure track is fp32 end to end (se3_modules.py:164): its input projections use the exact fp32 GEMM, also
        # under the "high" float32 matmul precision (exact=True)
        nin, Kp = _node_input(self, msa, seq_onehot, out_dtype=F32)
        wn = self.cached("wn32", lambda: torch.cat([self.node_embed[0].weight.detach().float(),
                                                    torch.zeros(self.node_embed[0].weight.shape[0],
                                                                Kp - self.node_embed[0].weight.shape[1],
                                                                device=msa.device)], 1).contiguous())
        node = ops.linear(nin, wn, _f(self.node_embed[0].bias), out_dtype=F32, act=L.ACT_ELU, exact=True)
        node = ln(self.node_embed[2], node, out_dtype=F32)
        e = ops.linear(ln(self.ln_pair, pair, out_dtype=F32), self.edge_embed[0].weight.detach().float(),
                       _f(self.edge_embed[0].bias), out_dtype=F32, act=L.ACT_ELU, exact=True)
        edge = ln(self.edge_embed[2], e, out_dtype=F32)  # [B,L,L,d_edge] fp32
        xyz = xyz.contiguous()
        g = build_graph(xyz, edge, aa_idx.contiguous(), self.n_neighbors, monotonic=monotonic)
        type0 = node.view(B * Lr, -1, 1)
        type1 = ops.center_ca(xyz).view(B * Lr, 3, 3)
        out = self.se3_transformer.run(g, type0, type1)
        state = out[0].view(B, Lr, -1)
        return state, ops.coord_apply(xyz, out[1].contiguous())

    def forward(self, xyz, msa, pair, aa_idx, seq_onehot):
        mono = check_index_range(None, None, aa_idx.contiguous(), 1, 2 ** 31 - 1)
        out = self.run(xyz.float(), msa.float().contiguous(), pair.float().contiguous(), aa_idx, seq_onehot.float(),
                       monotonic=mono)
        check_edge_capacity()
        return out


# ================================================================================================
# MSA update with coordinates
# ================================================================================================
class MsaUpdateWithPairAndCoord(RecordingModule):
    """rf.py:865-920.  enable_backward() (switches the FeedForward in `to_out` along): with grad mode on,
    forward(xyz, state, msa) records, and loss.backward() fills the .grad of every parameter of the module and of state and msa
    where they require grad.  xyz carries no gradient: it enters through the distance mask only, which is piecewise constant
    (xyz.grad stays None, as under the reference's autograd).  The backward walks the forward in reverse: the feed-forward
    (FeedForward._backward, its dropouts replayed in train() mode), ln_out, the attention . V contraction (d att and d v on
    rf_gemm), the map (rf_dist_masked_attention_bwd, include/rfmi.h), the three projections, and ln_state / ln_msa; LN(state),
    LN(msa), q, k, v^T and the 16-bit map are rebuilt from the saved inputs with the forward's own launches.  to_k.bias gets an
    exact zero: q_i . b_k is added to every logit of row i and drops out of the softmax (float64 autograd of the reference
    returns rounding noise for it, about 1e-15 of to_q.bias's gradient; a relative comparison against that is meaningless).
    The fp16 mode's power-of-two gradient scale is applied HERE, not by the autograd Function (_rf_scales_own_grads): the
    feed-forward, ln_out and the value path each run on a copy of their incoming gradient at a scale of their own; the q / k side
    is fp32 throughout and runs unscaled.  d_msa, d_msa / n_heads, d_state and n_heads * d_trfm_inner must be multiples of 8 while
    recording.  ThreeTrackBlock.run3, RoseTTAFold.forward and the captured graph call run() without a tape: they never record
    here."""
    _rf_n_inputs = 3   # xyz (no gradient), state, msa
    _rf_scales_own_grads = True

    def __init__(self, d_msa, d_state, d_trfm_inner, d_ff, distance_bins=[8, 12, 16, 20], p_dropout=0.1):
        super().__init__()
        self.distance_bins = distance_bins
        self.n_heads = len(distance_bins)
        self.d_inner = d_trfm_inner
        self.scale = (d_state // self.n_heads) ** -0.5  # rf.py:874
        self.ln_msa = LayerNorm(d_msa)
        self.ln_state = LayerNorm(d_state)
        self.to_q = Linear(d_state, d_trfm_inner * self.n_heads)
        self.to_k = Linear(d_state, d_trfm_inner * self.n_heads)
        self.to_v = Linear(d_msa, d_msa)
        self.ln_out = LayerNorm(d_msa)
        self.to_out = Residual(nn.Sequential(LayerNorm(d_msa), FeedForward(d_msa, d_ff, p_dropout)))

    @staticmethod
    def _map_dtype(Lr):
        """the type of the attention map and of the key-contiguous operands contracted with it over the chain"""
        return T() if Lr % 8 == 0 else F32

    def _attend(self, xyz, state, msa):
        """The forward up to the attention . V contraction; the backward rebuilds its operands with the same launches.  Returns
        (LN(state) fp32, LN(msa) fp32, LN(msa) T, scaled q fp32, k fp32, bins, the map [B,H,L,L], att . V fp32 [B,N,L,D]).  The map
        and v^T are of the compute type; in the 16-bit modes a chain length that is no multiple of 8, which the 16-bit GEMM cannot
        contract over (RF_EALIGN), keeps both in fp32 and contracts them on the exact fp32 kernel (_map_dtype)."""
        B, N, Lr, D = msa.shape
        H, dq = self.n_heads, self.d_inner
        dv = D // H
        dev = msa.device
        st = ln(self.ln_state, state.contiguous(), out_dtype=F32)
        m32 = ln(self.ln_msa, msa, out_dtype=F32)
        m_t = ops.cast(m32, T())
        q = ops.linear(st, self.to_q.weight.detach(), _f(self.to_q.bias), out_dtype=F32, exact=True)
        ops.axpby(q, self.scale, None, 0.0, q)
        k = ops.linear(st, self.to_k.weight.detach(), _f(self.to_k.bias), out_dtype=F32, exact=True)
        bins = self.cached("bins", lambda: torch.tensor(self.distance_bins, dtype=F32, device=dev))
        att = torch.empty(B, H, Lr, Lr, device=dev, dtype=self._map_dtype(Lr))
        ops.dist_masked_attention(q, k, xyz.contiguous(), bins, att, B, Lr, H, dq)
        v_t = torch.empty(B, N, D, Lr, device=dev, dtype=att.dtype)
        ops.gemm(self.wt("v", self.to_v), m_t, v_t, D, Lr, D, batch=(B * N, 1, 1), b_bs=(Lr * D, 0, 0),
                 c_bs=(D * Lr, 0, 0), c_row=(0, 0, Lr), bias=_f(self.to_v.bias), bias_mode=L.BIAS_ROW, exact=False)
        out = torch.empty(B, N, Lr, D, device=dev, dtype=F32)
        ops.gemm(att, v_t, out, Lr, N * dv, Lr, batch=(B, H, 1),
                 a_bs=(H * Lr * Lr, Lr * Lr, 0), a_row=(0, 0, Lr),
                 b_bs=(N * D * Lr, dv * Lr, 0), b_row=(dv, D * Lr, Lr),
                 c_bs=(N * Lr * D, dv, 0), c_row=(0, 0, D), c_col=(dv, Lr * D), exact=False)
        return st, m32, m_t, q, k, bins, att, out

    def run(self, xyz, state, msa, tape=None):
        """returns the new fp32 msa [B,N,L,D] (the residual base is LayerNorm(msa), rf.py:893,918).
        tape: a dict that receives what _backward needs (xyz, state, msa, an fp32 copy of the stream in front of the feed-forward
        and the feed-forward's own tape; same kernels, same numbers)."""
        D = msa.shape[-1]
        _check_backward_call(self, tape, None, D, D // self.n_heads, state.shape[-1], self.n_heads * self.d_inner)
        _, m32, _, _, _, _, _, out = self._attend(xyz, state, msa)
        o = ln(self.ln_out, out, out_dtype=F32)
        ops.axpby(m32, 1.0, o, 1.0, m32)
        sub = None
        if tape is not None:
            sub = {}
            tape.update(xyz=xyz, state=state, msa=msa, x1=_copy(m32), ff=sub)
        self.to_out.fn[1].apply_residual(ln(self.to_out.fn[0], m32), m32, tape=sub)
        return m32

    def _backward(self, tape, g):
        """g: contiguous fp32 [B, N, L, D] gradient of the output (overwritten).  Returns (fp32 d state [B, L, d_state], fp32
        d msa [B, N, L, D], {param: grad}).  With m = LN(msa), s = LN(state), x1 = m + LN_out(out), y = x1 + FF(LN_ff(x1)):
            g  <- g + d x1 of the feed-forward                           _pre_norm_residual_bwd; g is now d x1 = d m (residual) = d o
            d out, dgamma_o, dbeta_o = LayerNorm backward                rf_layernorm_bwd on the rebuilt att . V
            d att[b,h,i,j] = sum_{n,c} d out[b,n,i,h,c] v[b,n,j,h,c]     rf_gemm, K = N * dv in chunks of dv (v = to_v(m) row-major)
            d v[b,n,j,h,c] = sum_i att[b,h,i,j] d out[b,n,i,h,c]         rf_gemm: the forward's att . V call on the transposed
                                                                         16-bit map and d out^T
            dq', dk = rf_dist_masked_attention_bwd(q, k, xyz, d att);   dq = scale dq'
            dW_q, db_q = dq^T s, sum dq;   dW_k = dk^T s;   db_k = 0 exactly;   dW_v, db_v = dv^T m, sum dv     rf_conv_wgrad
            d s = dq W_q + dk W_k (exact fp32, like the forward);   d m = dv W_v + g                           rf_gemm
            d state, d msa and the two affines = LayerNorm backward                                          rf_layernorm_bwd
        In the fp16 mode the feed-forward, ln_out and the value path each run on a copy of their incoming gradient at a
        power-of-two scale of their own; d att is brought back to scale 1 in fp32 before the map's backward.  Every contraction of
        the backward is pinned exact (exact=True, like the sibling modules' input gradients): under the fp32 mode's "high" matmul
        precision the forward's value path follows it, the gradients stay on the exact fp32 kernel."""
        xyz, state, msa = tape["xyz"], tape["state"], tape["msa"]
        B, N, Lr, D = msa.shape
        H, dq_ = self.n_heads, self.d_inner
        dv = D // H
        dev = msa.device
        grads = {}
        _pre_norm_residual_bwd(g, self.to_out.fn[1]._backward, tape["ff"], tape["x1"], self.to_out.fn[0], grads)
        st, _, m_t, q, k, bins, att, out = self._attend(xyz, state, msa)
        # ---- ln_out
        s = _grad_scale([g])
        dout, dgo, dbo = ops.layernorm_bwd(out, _scaled_copy(g, s), _f(self.ln_out.weight), eps=self.ln_out.eps)
        del out
        gr = {self.ln_out.weight: dgo, self.ln_out.bias: dbo}
        _unscale([dout] + list(gr.values()), s)
        grads.update(gr)
        # ---- attention . V: d att and d v
        s = _grad_scale([dout])
        if s != 1.0:
            ops.axpby(dout, s, None, 0.0, dout)
        dout_t = ops.cast(dout, T())
        v = ops.linear(m_t, self.wt("v", self.to_v), _f(self.to_v.bias), exact=True)   # the values row-major: [B,N,L,D] T
        datt = torch.empty(B, H, Lr, Lr, device=dev, dtype=F32)
        ops.gemm(dout_t, v, datt, Lr, Lr, N * dv, batch=(B, H, 1), kc=dv,
                 a_bs=(N * Lr * D, dv, 0), a_row=(0, 0, D), a_ko=Lr * D,
                 b_bs=(N * Lr * D, dv, 0), b_row=(0, 0, D), b_ko=Lr * D,
                 c_bs=(H * Lr * Lr, Lr * Lr, 0), c_row=(0, 0, Lr), exact=True)
        del v
        _unscale([datt], s)
        dout_tt = torch.empty(B, N, D, Lr, device=dev, dtype=att.dtype)   # d out key-contiguous, like the forward's v^T
        ops.copy(dout_t.transpose(2, 3), dout_tt)
        att_tr = torch.empty(B, H, Lr, Lr, device=dev, dtype=att.dtype)
        ops.copy(att.transpose(2, 3), att_tr)
        del att, dout, dout_t
        dv_t = torch.empty(B, N, Lr, D, device=dev, dtype=att_tr.dtype)   # (fp32 where the map is: _map_dtype)
        ops.gemm(att_tr, dout_tt, dv_t, Lr, N * dv, Lr, batch=(B, H, 1),
                 a_bs=(H * Lr * Lr, Lr * Lr, 0), a_row=(0, 0, Lr),
                 b_bs=(N * D * Lr, dv * Lr, 0), b_row=(dv, D * Lr, Lr),
                 c_bs=(N * Lr * D, dv, 0), c_row=(0, 0, D), c_col=(dv, Lr * D), exact=True)
        del att_tr, dout_tt
        dv_t = ops.cast(dv_t, T())
        # ---- value projection, the residual path, ln_msa
        dwv, dbv = ops.conv_wgrad(dv_t, m_t, 1, bias=True)
        dm = ops.linear(dv_t, self.wt_input_grad("v", self.to_v), None, out_dtype=F32, exact=True)
        del dv_t, m_t
        gr = {self.to_v.weight: dwv, self.to_v.bias: dbv}
        _unscale([dm] + list(gr.values()), s)
        grads.update(gr)
        ops.axpby(dm, 1.0, g, 1.0, dm)
        dmsa, grads[self.ln_msa.weight], grads[self.ln_msa.bias] = ops.layernorm_bwd(msa, dm, _f(self.ln_msa.weight),
                                                                                     eps=self.ln_msa.eps)
        del dm
        # ---- the map, to_q / to_k, ln_state (fp32 throughout: no scale)
        dq, dk, _ = ops.dist_masked_attention_bwd(q, k, xyz.contiguous(), bins, datt, B, Lr, H, dq_)
        del datt
        ops.axpby(dq, self.scale, None, 0.0, dq)
        grads[self.to_q.weight], grads[self.to_q.bias] = ops.conv_wgrad(dq, st, 1, bias=True)
        grads[self.to_k.weight], _ = ops.conv_wgrad(dk, st, 1)
        grads[self.to_k.bias] = ops.zeros(H * dq_, device=dev, dtype=F32)
        wqt = self.cached("wqt32", lambda: self.to_q.weight.detach().float().t().contiguous())
        wkt = self.cached("wkt32", lambda: self.to_k.weight.detach().float().t().contiguous())
        dst = ops.linear(dq, wqt, None, out_dtype=F32, exact=True)
        ops.linear(dk, wkt, None, out=dst, residual=dst, exact=True)
        dstate, grads[self.ln_state.weight], grads[self.ln_state.bias] = ops.layernorm_bwd(
            state.contiguous(), dst, _f(self.ln_state.weight), eps=self.ln_state.eps)
        return dstate, dmsa, grads

    def _backward_children(self):
        return (self.to_out.fn[1],)

    def _record(self, xyz, state, msa, tape):
        return self.run(xyz.float(), state.float(), msa.float().contiguous(), tape=tape)

    def _backward_from_autograd(self, tape, gs, s, want):
        dstate, dmsa, grads = self._backward(tape, _scaled_copy(gs[0], 1.0))
        return (None, dstate.view(tape["state"].shape), dmsa), grads

    def forward(self, xyz, state, msa):
        if _recording(self):
            return _RecordedFn.apply(self, xyz, state, msa, *self.parameters())
        return self._record(xyz, state, msa, None)


# ================================================================================================
# blocks and model
# ================================================================================================
def _whole_pair(pair, row_group):
    """The whole pair tensor on every rank from the row blocks (identity without a row group)."""
    if row_group is None:
        return pair
    from . import shard
    return shard.all_gather_rows(pair, row_group)


class TwoTrackBlock(RFModule):
    """rf.py:923-968."""

    def __init__(self, d_msa, d_pair, n_encoder_layers, p_dropout=0.1):
        super().__init__()
        self.msa_update_using_self_att = MsaUpdateUsingSelfAttention(d_msa=d_msa, d_ff=d_msa * 4, n_heads=12,
                                                                     n_encoder_layers=n_encoder_layers,
                                                                     p_dropout=p_dropout)
        self.pair_update_with_msa = PairUpdateWithMsa(d_pair=d_pair, n_heads=12, d_msa=d_msa, d_proj=32)
        self.pair_update_with_axial_attention = PairUpdateWithAxialAttention(d_pair=d_pair, d_ff=d_pair * 4, n_heads=8,
                                                                            p_dropout=p_dropout,
                                                                            n_encoder_layers=n_encoder_layers,
                                                                            performer_kws={})
        self.msa_update_with_pair = MsaUpdateWithPair(d_msa=d_msa, d_pair=d_pair, n_heads=4,
                                                      n_encoder_layers=n_encoder_layers, p_dropout=p_dropout)

    def run(self, msa, pair, row_group=None):
        """msa updated in place; returns the new pair tensor.
        row_group: `pair` is this rank's block of rows shard_range(L, world, rank) of the pair tensor, msa is replicated
        (pair-track row-block sharding, shard.two_track_block_row_sharded): the MSA self-attention runs on every rank, the three
        pair-track modules run on the row block with their exchanges."""
        att = self.msa_update_using_self_att.run(msa)
        if row_group is None:
            pair = self.pair_update_with_msa.run(msa, pair, att)
            self.pair_update_with_axial_attention.run(pair)
            self.msa_update_with_pair.run(msa, pair)
            return pair
        pair = self.pair_update_with_msa.run_rows(msa, pair, att, row_group)
        self.pair_update_with_axial_attention.run(pair, row_group=row_group)
        self.msa_update_with_pair.run(msa, pair, row_group=row_group)
        return pair

    def forward(self, msa, pair):
        msa = fresh_f32(msa)
        pair = self.run(msa, pair.float().contiguous())
        return msa, pair


def _set_dropout(module, p):
    """Set every dropout probability below `module` (the nn.Dropout containers and the p_dropout fields the training-mode
    forward reads) -- the reference hard-codes 0.1 for the MsaUpdateWithPair of its three-track / final blocks."""
    for m in module.modules():
        if isinstance(m, nn.Dropout):
            m.p = p
        if getattr(m, "p_dropout", None) is not None:
            m.p_dropout = p


class ThreeTrackBlock(TwoTrackBlock):
    """rf.py:971-1046."""

    def __init__(self, d_msa, d_pair, d_node, d_edge, d_state, n_encoder_layers, n_neighbors, p_dropout):
        super().__init__(d_msa, d_pair, n_encoder_layers, p_dropout)
        _set_dropout(self.msa_update_with_pair, 0.1)   # rf.py:1015 (whatever the model's p_dropout)
        self.coord_update_with_msa_and_pair = CoordUpdateWithMsaAndPair(d_msa=d_msa, d_pair=d_pair, d_node=d_node,
                                                                        d_edge=d_edge, d_state=d_state,
                                                                        n_neighbors=n_neighbors, p_dropout=p_dropout)
        self.msa_update_with_pair_and_coord = MsaUpdateWithPairAndCoord(d_msa=d_msa, d_state=d_state, d_trfm_inner=32,
                                                                        d_ff=d_msa * 4, distance_bins=[8, 12, 16, 20],
                                                                        p_dropout=p_dropout)

    def run3(self, msa, pair, xyz, seq_onehot, aa_idx, monotonic=True, row_group=None):
        """row_group: `pair` is this rank's block of rows (TwoTrackBlock.run); the structure track runs replicated on the
        all-gathered pair tensor (it reads the pair rows of the kNN edges of every residue)."""
        pair = self.run(msa, pair, row_group)
        state, xyz = self.coord_update_with_msa_and_pair.run(xyz, msa, _whole_pair(pair, row_group), aa_idx, seq_onehot, monotonic)
        msa = self.msa_update_with_pair_and_coord.run(xyz, state, msa)
        return msa, pair, xyz

    def forward(self, msa, pair, xyz, seq_onehot, aa_idx):
        msa = fresh_f32(msa)
        mono = check_index_range(None, None, aa_idx.contiguous(), 1, 2 ** 31 - 1)
        out = self.run3(msa, pair.float().contiguous(), xyz.float(), seq_onehot.float(), aa_idx, mono)
        check_edge_capacity()
        return out


class FinalBlock(TwoTrackBlock):
    """rf.py:1049-1127."""

    def __init__(self, d_msa, d_pair, d_node, d_edge, d_state, n_encoder_layers, p_dropout, n_neighbors=32):
        super().__init__(d_msa, d_pair, n_encoder_layers, p_dropout)
        _set_dropout(self.msa_update_with_pair, 0.1)   # rf.py:1101
        self.coord_update_with_msa_and_pair = CoordUpdateWithMsaAndPair(d_msa=d_msa, d_pair=d_pair, d_node=d_node,
                                                                        d_edge=d_edge, d_state=d_state,
                                                                        n_neighbors=n_neighbors, p_dropout=p_dropout)
        self.plddt_head = Linear(d_state, 1)

    def run3(self, msa, pair, xyz, seq_onehot, aa_idx, monotonic=True, row_group=None, axial_grad=False):
        """axial_grad: the pair axial update records (its forward() under grad mode, enable_backward): the returned pair takes
        part in autograd; the MSA update and the structure track read a detached copy (the same numbers as the plain run)."""
        if axial_grad:
            att = self.msa_update_using_self_att.run(msa)
            pair = self.pair_update_with_msa.run(msa, pair, att)
            with torch.enable_grad():
                pair_rec = self.pair_update_with_axial_attention(pair)
            pair = pair_rec.detach()
            self.msa_update_with_pair.run(msa, pair)
        else:
            pair = self.run(msa, pair, row_group)
        state, xyz = self.coord_update_with_msa_and_pair.run(xyz, msa, _whole_pair(pair, row_group), aa_idx, seq_onehot, monotonic)
        plddt = ops.linear(state.contiguous(), self.plddt_head.weight.detach(), _f(self.plddt_head.bias), out_dtype=F32, exact=True)
        return msa, (pair_rec if axial_grad else pair), xyz, plddt[..., 0]

    def forward(self, msa, pair, xyz, seq_onehot, aa_idx):
        msa = fresh_f32(msa)
        mono = check_index_range(None, None, aa_idx.contiguous(), 1, 2 ** 31 - 1)
        out = self.run3(msa, pair.float().contiguous(), xyz.float(), seq_onehot.float(), aa_idx, mono)
        check_edge_capacity()
        return out


class RoseTTAFold(RFModule):
    """rf.py:1175-1289: RoseTTAFold(msa, seq, aa_idx) -> (logits dict, xyz [B,L,3,3], plddt [B,L])."""

    def __init__(self, d_input=21, d_msa=384, d_pair=288, d_node=64, d_edge=64, d_state=32, n_two_track_blocks=3,
                 n_three_track_blocks=4, n_encoder_layers=4, max_len=5000, n_neighbors=[128, 128, 64, 64, 64],
                 p_dropout=0.1, use_template=False):
        super().__init__()
        self.d_msa, self.d_pair, self.d_node, self.d_edge, self.d_state = d_msa, d_pair, d_node, d_edge, d_state
        self.n_two_track_blocks, self.n_three_track_blocks = n_two_track_blocks, n_three_track_blocks
        self.n_encoder_layers, self.use_template = n_encoder_layers, use_template
        self.msa_emb = MsaEmbedding(d_input=d_input, d_msa=d_msa, max_len=max_len, p_pe_drop=p_dropout)
        self.pair_emb = PairEmbedding(d_input=d_input, d_pair=d_pair, max_len=max_len, use_template=use_template,
                                      p_pe_drop=p_dropout)
        self.two_track_blocks = nn.ModuleList([TwoTrackBlock(d_msa, d_pair, n_encoder_layers=n_encoder_layers,
                                                             p_dropout=p_dropout) for _ in range(n_two_track_blocks)])
        self.initial_coord_generation_with_msa_and_pair = InitialCoordGenerationWithMsaAndPair(
            d_msa=d_msa, d_pair=d_pair, d_node=d_node, d_edge=d_edge, n_heads=4, n_layers=4, p_dropout=p_dropout)
        self.three_track_blocks = nn.ModuleList([
            ThreeTrackBlock(d_msa, d_pair, d_node, d_edge, d_state, n_encoder_layers=n_encoder_layers,
                            n_neighbors=n_neighbors[i], p_dropout=p_dropout) for i in range(n_three_track_blocks - 1)])
        self.final_block = FinalBlock(d_msa, d_pair, d_node, d_edge, d_state, n_encoder_layers=n_encoder_layers,
                                      n_neighbors=32, p_dropout=p_dropout)
        self.prediction_head = PredictionHead(in_channels=d_pair, n_res_blocks=4, p_dropout=p_dropout)

    def forward(self, msa, seq, aa_idx):
        """The inference forward, under no_grad.  With prediction_head.enable_backward() and the caller's grad mode on, the trunk
        still runs under no_grad and only the head records: the logits take part in autograd (xyz and plddt do not).
        With final_block.pair_update_with_axial_attention.enable_backward() as well, that update records too (the trunk runs
        under no_grad up to its input; its output feeds the recording head, a detached copy the MSA update and the structure
        track), so the gradient reaches its parameters.  It needs the head: enabling it alone raises ValueError.  The axial
        updates of the two-track and three-track blocks record only when called directly, never inside this forward."""
        head_grad = _recording(self.prediction_head)
        axial_grad = _recording(self.final_block.pair_update_with_axial_attention)
        if axial_grad and not head_grad:
            raise ValueError("final_block.pair_update_with_axial_attention has backward enabled but prediction_head does not: no "
                             "gradient could reach it (enable_backward() on the head too)")
        with torch.no_grad():
            if not msa.is_cuda:
                raise L.RfmiError("RoseTTAFold (MI355X build) needs device tensors; there is no CPU fallback")
            with torch.cuda.device(msa.device):  # device guard: kernels go to the inputs' GPU, whatever the caller's current one
                msa, seq, aa_idx = msa.contiguous(), seq.contiguous(), aa_idx.contiguous()
                # the reference raises IndexError for out-of-range tokens / residue indices (nn.Embedding, rf.py:73,98)
                mono = check_index_range(msa, seq, aa_idx, self.msa_emb.to_embedding.num_embeddings,
                                         min(self.msa_emb.pos_enc.max_len, self.pair_emb.pos_enc.max_len))
                _PENDING_EDGE_COUNTS.clear()
                if not head_grad:
                    out = self.forward_validated(msa, seq, aa_idx, mono)
                    check_edge_capacity()
                    return out
                p, xyz, plddt = self._trunk(msa, seq, aa_idx, mono, axial_grad=axial_grad)
                check_edge_capacity()
        with torch.cuda.device(msa.device), torch.enable_grad():
            logits = self.prediction_head(p)
        return logits, xyz, plddt

    @torch.no_grad()
    def forward_validated(self, msa, seq, aa_idx, mono=True, row_group=None):
        """forward() behind the input validation: launches only, no host read of device data, so it can be recorded into
        a hipGraph (graph.GraphedForward).  `mono` = aa_idx strictly increasing in every sample (what forward() checks).
        row_group: ONE sample spread over the ranks of a torch.distributed group (shard.forward_row_sharded): every rank gets the
        same inputs, the pair track runs on row blocks shard_range(L, world, rank), the MSA and structure tracks are replicated;
        returns this rank's rows of the logit maps and the whole xyz / plddt."""
        with torch.cuda.device(msa.device):
            p, xyz, plddt = self._trunk(msa, seq, aa_idx, mono, row_group)
            logits = self.prediction_head.run(p, row_group)
        return logits, xyz, plddt

    @torch.no_grad()
    def _trunk(self, msa, seq, aa_idx, mono, row_group=None, axial_grad=False):
        """forward_validated up to the prediction head: returns (pair or this rank's rows of it, xyz, plddt).  axial_grad: the
        final block's pair axial update records (FinalBlock.run3)."""
        with torch.cuda.device(msa.device):
            m = self.msa_emb.run(msa, aa_idx)
            p = self.pair_emb.run(seq, aa_idx)
            if row_group is not None:
                from . import shard
                p = shard.take_rows(p, row_group)
            onehot = ops.onehot(seq, 21)  # rf.py:1276
            for blk in self.two_track_blocks:
                p = blk.run(m, p, row_group)
            xyz = self.initial_coord_generation_with_msa_and_pair.run(m, _whole_pair(p, row_group), onehot, aa_idx)
            for blk in self.three_track_blocks:
                m, p, xyz = blk.run3(m, p, xyz, onehot, aa_idx, mono, row_group)
            m, p, xyz, plddt = self.final_block.run3(m, p, xyz, onehot, aa_idx, mono, row_group, axial_grad=axial_grad)
        return p, xyz, plddt


def flat_state(model):
    """state_dict as fp32 CPU tensors (the form the CPU oracle consumes)."""
    return {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
