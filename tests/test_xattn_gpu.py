"""mm_xattn_* (csrc/mm_xattn.hip): the core of `CrossAttention` (reference model/attention.py:79-96) at the head widths the reference's
MoE recipes use (cookbook/sft/moe/*/attn/shared: 768 / 8 = 96; .../attn/pep: 4096 / 8 = 512) and a few others, forward + backward,
with and without attention-probability dropout, against a plain torch restatement run in float64 on the SAME bf16 / fp32 operands.

Dropout: torch's generator cannot be reproduced draw for draw, so train mode is "parity unpinned" against the reference; what is
held here: (a) with the kernels' own keep mask (mm_dropout_mask lists it) the outputs and gradients equal the torch restatement
(bf16 <= 2e-2, fp32 <= 1e-4), (b) the keep rate is 1 - p within 4 sigma, (c) p = 0 is bit-identical to the eval path, (d) same
(seed, offset) -> same bits, another offset -> another mask, (e) the fp32 and bf16 kernels drop the same elements."""
import math

import pytest
import torch

from tests.xattn_check import dropout_keep, keep_mask

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _mask(K, seed, off, n, H, Nq, Nkv, p):
    KP = (Nkv + 31) // 32 * 32
    m = K.dropout_mask(seed, off, n * H * Nq * KP, p)
    return m.view(n, H, Nq, KP)[..., :Nkv].to(torch.float64)


def _ref(q, k, v, do, scale, mask, p):
    """float64 restatement of attention.py:79-96 on [n, N, H, D] operands with a given keep mask [n, H, Nq, Nkv]."""
    q, k, v = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    pr = torch.softmax(s, dim=-1)
    if mask is not None:
        pr = pr * mask / (1.0 - p)
    o = torch.einsum("bhqk,bkhd->bqhd", pr, v)
    o.backward(do.double())
    return o.detach(), q.grad, k.grad, v.grad


def _operands(n, Nq, Nkv, H, D, dtype, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    C = H * D
    q2d = torch.randn(n * Nq, C, device="cuda", generator=g).to(dtype)
    kv2d = torch.randn(n * Nkv, 2 * C, device="cuda", generator=g).to(dtype)          # k | v as the fused projection leaves them
    do = torch.randn(n, Nq, H, D, device="cuda", generator=g).to(dtype)
    q = q2d.view(n, Nq, H, D)
    k = kv2d[:, :C].view(n, Nkv, H, D)
    v = kv2d[:, C:].view(n, Nkv, H, D)
    return q2d, kv2d, q, k, v, do


SHAPES = [  # n, Nq, Nkv, H, D
    (2, 49, 196, 8, 96),      # shared-projector recipe: ViT-B/32 experts, C = 768, 8 heads, P = 49, E = 5
    (2, 49, 196, 8, 512),     # per-expert-projection recipe: C = 4096, 8 heads
    (3, 16, 64, 2, 64),       # the reference-generated fixture's geometry (tests/golden/tiny_moe_clip)
    (1, 70, 33, 3, 72),       # two query tiles, ragged keys, a head width that is no multiple of 16
    (1, 130, 500, 2, 128),    # three query tiles, the 32-tile instantiation
    (2, 5, 7, 1, 8),          # tiny
    (1, 256, 1024, 2, 96),    # round 4: up to 1024 keys (4 ViT-L/14 experts x 256 patches) in the 64-tile instantiation, dropout inside
    (1, 256, 1024, 1, 512),   # ... at the per-expert-projection recipe's head width
    (1, 70, 777, 2, 96),      # ... ragged
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_xattn_matches_float64_restatement(shape, dtype, p):
    from multimeditron_amd import kernels as K
    n, Nq, Nkv, H, D = shape
    q2d, kv2d, q, k, v, do = _operands(n, Nq, Nkv, H, D, dtype)
    scale = D ** -0.5
    seed, off = 1234, 7
    out, lse = K.xattn_fwd(q, k, v, scale, p, seed, off)
    dq2d, dkv2d = torch.full_like(q2d, float("nan")), torch.full_like(kv2d, float("nan"))
    C = H * D
    K.xattn_bwd(q, k, v, out, do, lse, scale, p, seed, off, dq2d.view(n, Nq, H, D), dkv2d[:, :C].view(n, Nkv, H, D),
                dkv2d[:, C:].view(n, Nkv, H, D))
    torch.cuda.synchronize()
    mask = _mask(K, seed, off, n, H, Nq, Nkv, p) if p > 0 else None
    if p > 0:       # the mask the kernels list is the documented one (tests/xattn_check.py computes it on the CPU)
        assert torch.equal(mask.bool().cpu(), keep_mask(seed, off, n, H, Nq, Nkv, p))
    o_ref, dq_ref, dk_ref, dv_ref = _ref(q, k, v, do, scale, mask, p)
    tol = 2e-2 if dtype == torch.bfloat16 else 1e-4
    assert torch.isfinite(dq2d.float()).all() and torch.isfinite(dkv2d.float()).all()          # every gradient element was written
    assert rel(out, o_ref) < tol
    assert rel(dq2d.view(n, Nq, H, D), dq_ref) < tol
    assert rel(dkv2d[:, :C].view(n, Nkv, H, D), dk_ref) < tol
    assert rel(dkv2d[:, C:].view(n, Nkv, H, D), dv_ref) < tol
    # lse = logsumexp of the scaled scores (dropout does not enter it)
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * scale
    assert rel(lse, torch.logsumexp(s, dim=-1)) < (5e-3 if dtype == torch.bfloat16 else 1e-5)


def test_xattn_p0_equals_eval_and_is_deterministic():
    from multimeditron_amd import kernels as K
    n, Nq, Nkv, H, D = 2, 49, 196, 8, 96
    q2d, kv2d, q, k, v, do = _operands(n, Nq, Nkv, H, D, torch.bfloat16)
    a, _ = K.xattn_fwd(q, k, v, D ** -0.5, 0.0, 1, 1)
    b, _ = K.xattn_fwd(q, k, v, D ** -0.5, 0.0, 99, 5)          # p = 0: the stream is never consulted
    assert torch.equal(a, b)
    c1, _ = K.xattn_fwd(q, k, v, D ** -0.5, 0.1, 42, 3)
    c2, _ = K.xattn_fwd(q, k, v, D ** -0.5, 0.1, 42, 3)
    c3, _ = K.xattn_fwd(q, k, v, D ** -0.5, 0.1, 42, 4)
    assert torch.equal(c1, c2) and not torch.equal(c1, c3) and not torch.equal(c1, a)


def test_xattn_bf16_and_fp32_drop_the_same_elements():
    from multimeditron_amd import kernels as K
    n, Nq, Nkv, H, D = 1, 49, 196, 2, 96
    q2d, kv2d, q, k, v, do = _operands(n, Nq, Nkv, H, D, torch.bfloat16)
    ob, _ = K.xattn_fwd(q, k, v, D ** -0.5, 0.25, 5, 11)
    of, _ = K.xattn_fwd(q.float(), k.float().contiguous(), v.float().contiguous(), D ** -0.5, 0.25, 5, 11)
    assert rel(ob, of) < 2e-2                                   # different masks would differ by ~ sqrt(p / (1 - p))


def test_dropout_keep_rate_and_adjoint():
    from multimeditron_amd import kernels as K
    p, N = 0.1, 1 << 20
    m = K.dropout_mask(7, 3, N, p).float()
    rate = float(m.mean())
    assert abs(rate - (1 - p)) < 4 * math.sqrt(p * (1 - p) / N), rate
    assert not torch.equal(m, K.dropout_mask(7, 4, N, p).float()) and not torch.equal(m, K.dropout_mask(8, 3, N, p).float())
    for dtype in (torch.bfloat16, torch.float32):
        x = torch.randn(1000, 77, device="cuda").to(dtype)       # 77000 elements: not a multiple of 4
        y = K.dropout(x, p, 7, 3)
        keep = K.dropout_mask(7, 3, x.numel(), p).view_as(x).bool()
        assert torch.equal(keep.cpu().view(-1), dropout_keep(7, 3, x.numel(), p))
        want = torch.where(keep, (x.float() / (1 - p)), torch.zeros((), device="cuda")).to(dtype)
        assert torch.equal(y, want)


def _pack(module):
    from multimeditron_amd.nn import FlatParams
    FlatParams([(k, p, "encoder") for k, p in module.named_parameters()], "cuda", torch.bfloat16)      # k|v weights adjacent: one GEMM
    return module


def test_cross_attention_module_dropout_semantics():
    """nn.Dropout semantics of the module: eval -> no dropout (deterministic), train -> both dropouts act, backward reuses the masks."""
    from multimeditron_amd.model.modalities.image_modality_moe import CrossAttention
    torch.manual_seed(0)
    ca = CrossAttention(768, num_heads=8, qkv_bias=True, dtype=torch.bfloat16, device="cuda")
    for prm in ca.parameters():
        torch.nn.init.normal_(prm, std=0.02)
    _pack(ca)
    x = torch.randn(4, 49, 768, device="cuda").to(torch.bfloat16)
    ctx = torch.randn(4, 196, 768, device="cuda").to(torch.bfloat16)
    ca.eval()
    with torch.no_grad():
        e1, e2 = ca(x, ctx), ca(x, ctx)
    assert torch.equal(e1, e2)
    ca.train()
    with torch.no_grad():
        t1, t2 = ca(x, ctx), ca(x, ctx)
    assert not torch.equal(t1, t2) and not torch.equal(t1, e1)
    zeros = float((t1 == 0).float().mean())                      # proj_drop zeroes ~10 % of the outputs
    assert 0.07 < zeros < 0.13, zeros
    xg = x.clone().requires_grad_(True)
    y = ca(xg, ctx)
    y.float().square().sum().backward()
    assert torch.isfinite(xg.grad.float()).all() and float(xg.grad.float().abs().sum()) > 0
    assert all(prm.grad is not None for prm in ca.parameters())


@pytest.mark.parametrize("dim", [768, 4096])
def test_cross_attention_recipe_geometry_vs_float64(dim):
    """CrossAttention at the shipped recipes' geometry (P = 49 queries, E - 1 = 4 specialists, 8 heads of 96 / 512), eval mode,
    bf16 kernels against a float64 restatement of attention.py:48-101 on the same bf16-rounded weights."""
    from multimeditron_amd.model.modalities.image_modality_moe import CrossAttention
    torch.manual_seed(1)
    n, P, E, h = 4, 49, 5, 8
    ca = CrossAttention(dim, num_heads=h, qkv_bias=True, dtype=torch.bfloat16, device="cuda").eval()
    for prm in ca.parameters():
        torch.nn.init.normal_(prm, std=dim ** -0.5)
    _pack(ca)
    x = torch.randn(n, P, dim, device="cuda").to(torch.bfloat16)
    ctx = torch.randn(n, (E - 1) * P, dim, device="cuda").to(torch.bfloat16)
    xg, cg = x.clone().requires_grad_(True), ctx.clone().requires_grad_(True)
    y = ca(xg, cg)
    dy = torch.randn_like(y)
    y.backward(dy)
    w = {k: v.detach().double() for k, v in ca.named_parameters()}
    xd, cd = x.double().requires_grad_(True), ctx.double().requires_grad_(True)
    lin = lambda t, nm: t @ w[nm + ".weight"].t() + w[nm + ".bias"]
    d = dim // h
    q = lin(xd, "q_proj").view(n, P, h, d).transpose(1, 2)
    k = lin(cd, "k_proj").view(n, -1, h, d).transpose(1, 2)
    v = lin(cd, "v_proj").view(n, -1, h, d).transpose(1, 2)
    att = torch.softmax(q @ k.transpose(-2, -1) * d ** -0.5, dim=-1)
    ref = lin((att @ v).transpose(1, 2).reshape(n, P, dim), "proj")
    ref.backward(dy.double())
    assert rel(y, ref) < 3e-2
    assert rel(xg.grad, xd.grad) < 6e-2 and rel(cg.grad, cd.grad) < 6e-2
