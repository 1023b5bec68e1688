"""rf_dist_masked_attention_bwd (csrc/backward.hip): the backward of MsaUpdateWithPairAndCoord's distance-masked attention map.

The kernel is held against float64 autograd of a restatement of the forward on the operands, by the yardstick rule of
tests/grad_oracle.py, with 2^-24, the rounding unit of the fp32 outputs.  A row is one (b, i) of dq, one (b, j) of dk.

Coordinates are a random walk of 3.8 A steps for CA plus unit noise for the other two atoms.  Before any launch each case
asserts on the CPU that every pairwise CA distance is at least 1e-4 A away from every bin (the fp32 distance error at these
ranges is about 1e-5, so the float64 mask is the kernel's) and, for L >= 24, that every head of every sample has both masked and
unmasked entries off the diagonal.

RF_MSA_COORD_BACKWARD_ERRORS=FILE: the measured errors are also merged into that JSON file (key "kernel_errors")."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import grad_oracle as G  # noqa: E402
import rosettafold_pytorch_amd as R  # noqa: E402
from rosettafold_pytorch_amd import _lib, ops  # noqa: E402

DEV = "cuda"
BINS4 = (8.0, 12.0, 16.0, 20.0)
# (B, L, H, d) -> bins.  L = 1: everything exactly zero; 63 / 65 / 100 / 257: below and above one and four trips of a wave's 64
# lanes; H = 5: a second trip of the per-wave head loop; d = 24: no power of two, and H * d = 120 is no multiple of the 16
# channels a lane group takes; 257 x 4 logits cross the 256 threads of a block more than four times.
SHAPES = {(2, 1, 4, 32): BINS4, (1, 5, 4, 32): BINS4, (2, 24, 4, 32): BINS4, (1, 63, 1, 8): (12.0,),
          (1, 65, 5, 24): (6.0, 8.0, 12.0, 16.0, 20.0), (1, 100, 4, 32): BINS4, (1, 257, 4, 32): BINS4}
SEED = {**{s: 0 for s in SHAPES}, (2, 24, 4, 32): 5}   # (seed 5: the 20 A head has entries out of range in both samples)
GAP = 1e-4
NAMES = ("dq", "dk")
RECORDS = []
HELD = dict(units=G.UNIT[torch.float32], rows=1, records=RECORDS)
_restore_mode = G.restore_mode()
_write_records = G.records_fixture("RF_MSA_COORD_BACKWARD_ERRORS", RECORDS, "max(torch float32 autograd vs float64, 2^-24)")


@pytest.fixture(params=[torch.bfloat16, torch.float16], ids=["bf16-build", "f16-build"])
def build(request):
    """the kernel takes fp32 operands only, and is built into both libraries"""
    R.set_compute_dtype(request.param)
    return request.param


def coordinates(B, L, g_):
    """fp32 [B, L, 3, 3]: CA (atom 1) a random walk of 3.8 A steps, N and C at unit noise around it"""
    step = torch.randn(B, L, 3, generator=g_)
    ca = (3.8 * step / step.norm(dim=-1, keepdim=True)).cumsum(1)
    return (ca[:, :, None, :] + torch.randn(B, L, 3, 3, generator=g_) * torch.tensor([1.0, 0.0, 1.0])[:, None]).float().contiguous()


def in_range(xyz, bins):
    """the float64 mask [B, H, L, L] of fp32 coordinates (True: within the head's bin), and the smallest gap to a bin"""
    ca = xyz[:, :, 1].double()
    dist = (ca[:, :, None] - ca[:, None]).norm(dim=-1)
    b_ = torch.tensor(bins, dtype=torch.float64)
    gap = (dist[:, None] - b_[None, :, None, None]).abs().min().item()
    return dist[:, None] < b_[None, :, None, None], gap


def preconditions(xyz, bins):
    """asserted on the CPU before any launch; returns the float64 mask"""
    mask, gap = in_range(xyz, bins)
    assert gap >= GAP, f"a CA distance lies {gap:.2e} A from a bin: choose another seed"
    L = xyz.shape[1]
    if L >= 24:
        off = ~torch.eye(L, dtype=torch.bool)
        per_head = lambda m: (m & off).transpose(0, 1).flatten(1).any(-1).all()   # noqa: E731
        assert per_head(mask) and per_head(~mask), "a head is all in or all out of range"
    return mask


@functools.lru_cache(maxsize=None)
def case(shape):
    """One set of operands per shape, shared by the tests below and left unchanged."""
    B, L, H, d = shape
    g_ = torch.Generator().manual_seed(4100 + SEED[shape])
    xyz = coordinates(B, L, g_)
    mask = preconditions(xyz, SHAPES[shape])
    q = torch.randn(B, L, H * d, generator=g_) * d ** -0.25    # logits of unit scale: q arrives pre-scaled
    k = torch.randn(B, L, H * d, generator=g_) * d ** -0.25
    datt = torch.randn(B, H, L, L, generator=g_)
    return dict(q=q.to(DEV), k=k.to(DEV), xyz=xyz.to(DEV), bins=torch.tensor(SHAPES[shape], dtype=torch.float32, device=DEV),
                datt=datt.to(DEV), mask=mask, shape=shape)


def autograd(c, dtype, mask=None):
    """the forward restated on the operands (rf.py:899-914) and differentiated by torch: sum(softmax_j(q.k + bias) * datt)"""
    B, L, H, d = c["shape"]
    q, k = (c[n].detach().cpu().to(dtype).clone().requires_grad_() for n in ("q", "k"))
    mask = c["mask"] if mask is None else mask
    bias = torch.where(mask, 0.0, -1e9).to(dtype)
    logit = torch.einsum("bihc,bjhc->bhij", q.view(B, L, H, d), k.view(B, L, H, d)) + bias
    (logit.softmax(-1) * c["datt"].cpu().to(dtype)).sum().backward()
    return {"dq": q.grad, "dk": k.grad}


@functools.lru_cache(maxsize=None)
def refs(shape):
    c = case(shape)
    return autograd(c, torch.float64), autograd(c, torch.float32)


def run_bwd(c, **over):
    t = dict(c, **over)
    B, L, H, d = t["shape"]
    dq, dk, ds = ops.dist_masked_attention_bwd(t["q"], t["k"], t["xyz"], t["bins"], t["datt"], B, L, H, d)
    return {"dq": dq, "dk": dk, "ds": ds}


# ---- 1. the kernel against float64 autograd ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES), ids=[str(s) for s in SHAPES])
def test_kernel_against_float64_autograd(shape, build):
    c = case(shape)
    ref64, ref32 = refs(shape)
    got = run_bwd(c)
    B, L, H, d = shape
    for n in NAMES:
        assert got[n].dtype == torch.float32 and tuple(got[n].shape) == (B, L, H * d)
    tag = f"{'bf16' if build == torch.bfloat16 else 'f16'}-build {shape}"
    assert G.held(got, ref64, ref32, tag, **HELD)
    # a masked entry has p = 0, and so ds = 0, exactly; the float64 mask is the kernel's
    assert (got["ds"].cpu()[~c["mask"]] == 0).all()
    if L == 1:
        assert (got["dq"] == 0).all() and (got["dk"] == 0).all() and (got["ds"] == 0).all()
    if L >= 5:   # the check has teeth: the gradient of the transposed map must fail it
        wrong = run_bwd(c, datt=c["datt"].transpose(-1, -2).contiguous())
        assert not G.held(wrong, ref64, ref32, f"{tag} (transposed gradient: must fail)", **HELD)
        del RECORDS[-len(NAMES):]


# ---- 2. exact facts ------------------------------------------------------------------------------------------------------------
def test_a_residue_out_of_range_gets_exact_zeros():
    """one residue moved 1000 A away attends to itself alone (p = 1) and nobody attends to it (p = 0): its row of dq and its
    row of dk are exactly zero; the others still match float64 autograd under the moved mask"""
    shape, r = (2, 24, 4, 32), 5
    c = dict(case(shape))
    xyz = c["xyz"].clone()
    xyz[:, r] += 1000.0
    mask, gap = in_range(xyz.cpu(), SHAPES[shape])
    assert gap >= GAP
    assert not mask[:, :, r, :r].any() and not mask[:, :, r, r + 1:].any() and not mask[:, :, :r, r].any()
    c.update(xyz=xyz, mask=mask)
    got = run_bwd(c)
    assert (got["dq"][:, r] == 0).all() and (got["dk"][:, r] == 0).all()
    assert (got["dq"][:, r + 1] != 0).any() and (got["dk"][:, r + 1] != 0).any()
    assert G.held(got, autograd(c, torch.float64), autograd(c, torch.float32), f"{shape} residue {r} moved 1000 A", **HELD)
    del RECORDS[-len(NAMES):]


@pytest.mark.parametrize("shape", [(1, 65, 5, 24), (1, 257, 4, 32)], ids=str)
def test_two_calls_give_the_same_bits(shape, build):
    c = case(shape)
    a, b = run_bwd(c), run_bwd(c)
    assert all(torch.equal(a[n], b[n]) for n in a)


def test_inputs_and_guard_bands_are_untouched():
    R.set_compute_dtype(torch.bfloat16)
    shape = (1, 65, 5, 24)
    B, L, H, d = shape
    c = case(shape)
    plain = run_bwd(c)
    keep = {n: c[n].clone() for n in ("q", "k", "xyz", "bins", "datt")}
    G = 64   # guard elements on each side
    bufs = {"dq": B * L * H * d, "dk": B * L * H * d, "ds": B * H * L * L}
    mem = {n: torch.full((G + sz + G,), -7.0, device=DEV) for n, sz in bufs.items()}
    rc = _lib.lib.rf_dist_masked_attention_bwd(ops.ptr(c["q"]), ops.ptr(c["k"]), ops.ptr(c["xyz"]), ops.ptr(c["bins"]),
                                               ops.ptr(c["datt"]), ops.ptr(mem["dq"], G), ops.ptr(mem["dk"], G), ops.ptr(mem["ds"], G),
                                               B, L, H, d, ops.stream())
    assert rc == 0
    torch.cuda.synchronize()
    for n, sz in bufs.items():
        assert (mem[n][:G] == -7).all() and (mem[n][G + sz:] == -7).all(), n
        assert torch.equal(mem[n][G:G + sz], plain[n].reshape(-1)), n   # every element written, the same bits
    for n, t in keep.items():
        assert torch.equal(c[n], t), n


def test_entry_point_refuses_before_a_launch():
    R.set_compute_dtype(torch.bfloat16)
    B, L, H, d = 1, 4, 2, 8
    q, k = torch.zeros(B, L, H * d, device=DEV), torch.zeros(B, L, H * d, device=DEV)
    xyz, bins = torch.zeros(B, L, 3, 3, device=DEV), torch.ones(H, device=DEV)
    datt, ds = torch.zeros(B, H, L, L, device=DEV), torch.zeros(B, H, L, L, device=DEV)
    dq, dk = torch.zeros_like(q), torch.zeros_like(k)
    p_ = ops.ptr

    def call(q_=q, k_=k, xyz_=xyz, bins_=bins, datt_=datt, dq_=dq, dk_=dk, ds_=ds, B_=B, L_=L, H_=H, d_=d):
        return _lib.lib.rf_dist_masked_attention_bwd(p_(q_), p_(k_), p_(xyz_), p_(bins_), p_(datt_), p_(dq_), p_(dk_), p_(ds_),
                                                     B_, L_, H_, d_, ops.stream())

    assert call() == 0
    for name in ("q_", "k_", "xyz_", "bins_", "datt_", "dq_", "dk_", "ds_"):   # RF_EINVAL: a NULL tensor
        assert call(**{name: None}) == -1, name
    for name in ("B_", "L_", "H_", "d_"):
        assert call(**{name: 0}) == -1, name
    # H * L * 4 bytes of LDS > 64 KB, the forward's own limit: refused, nothing launched (the tensors are far too small)
    assert call(L_=16385, H_=1) == -1
    assert call(L_=4097, H_=4) == -1
    att = torch.empty(1, device=DEV, dtype=torch.bfloat16)
    assert _lib.lib.rf_dist_masked_attention(p_(q), p_(k), p_(xyz), p_(bins), p_(att), _lib.RF_BF16, 1, 4097, 4, d, ops.stream()) == -1
    torch.cuda.synchronize()
    with pytest.raises(ValueError):   # the wrapper's own checks
        ops.dist_masked_attention_bwd(q, k, xyz, bins, datt[:, :1], B, L, H, d)
    with pytest.raises(ValueError):
        ops.dist_masked_attention_bwd(q, k, xyz[:, :2], bins, datt, B, L, H, d)
