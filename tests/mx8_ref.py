"""fp64 restatement of CausalLM.forward(..., prefill_weights="mxfp8") in torch: the decoder layer's own maths (RMSNorm, q|k|v with
bias, per-head q/k norm, RoPE with rotate_half, causal grouped-query attention, SwiGLU or xIELU, the two residuals, the final norm,
lm_head) with the MXFP8 format of tests/w8_check.py applied where the GPU path applies it: to the bf16-rounded input of each of
the four linears and to their weights.  Everything else stays fp64, so the distance of the GPU logits to this reference is the
GPU path's own rounding (bf16 between kernels, fp32 inside them), not the format's error."""
import torch

from tests import w8_check as W8


def qdq(t):
    """a GEMM operand as the MXFP8 path sees it: rounded to bf16 (it is a bf16 tensor when it reaches its linear), quantised,
    dequantised"""
    return W8.roundtrip_ref(t.to(torch.bfloat16).cpu()).double().to(t.device)


def rmsnorm(x, w, eps):
    return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * w.double()


def rope(x, cos, sin):
    """x [T, heads, D]; cos / sin [T, D/2]"""
    h = x.shape[-1] // 2
    lo, hi = x[..., :h], x[..., h:]
    c, s = cos[:, None, :], sin[:, None, :]
    return torch.cat([lo * c - hi * s, hi * c + lo * s], -1)


def xielu(x, alpha_p_raw, alpha_n_raw, beta, eps):
    sp = torch.nn.functional.softplus
    ap, an = sp(alpha_p_raw.double()), beta + sp(alpha_n_raw.double())
    return torch.where(x > 0, ap * x * x + beta * x, (torch.expm1(torch.minimum(x, torch.full_like(x, eps))) - x) * an + beta * x)


@torch.no_grad()
def forward(m, ids):
    """logits [B, S, V] in fp64 of the CausalLM m on ids [B, S] (no padding, positions 0 .. S-1)."""
    cfg = m.config
    B, S = ids.shape
    H, D = cfg.hidden_size, cfg.head_dim
    dev = ids.device
    x = m.model.embed_tokens.weight.data.double()[ids.reshape(-1)]
    pos = torch.arange(S, device=dev).unsqueeze(0).expand(B, S)
    cos, sin = (t.double() for t in m._tables(pos))
    causal = torch.ones(S, S, dtype=torch.bool, device=dev).tril()
    for layer in m.model.layers:
        a, ml = layer.self_attn, layer.mlp
        Hq, Hkv = a.Hq, a.Hkv
        n1, n2 = layer.norms()
        h = rmsnorm(x, n1.weight.data, n1.eps)
        qkv = qdq(h) @ qdq(a._wqkv.tensor()).t()
        if a._bqkv is not None:
            qkv = qkv + a._bqkv.tensor().double()
        q = qkv[:, : Hq * D].view(B * S, Hq, D)
        k = qkv[:, Hq * D:(Hq + Hkv) * D].view(B * S, Hkv, D)
        v = qkv[:, (Hq + Hkv) * D:].view(B, S, Hkv, D)
        if a.q_norm is not None:
            q, k = rmsnorm(q, a.q_norm.weight.data, a.q_norm.eps), rmsnorm(k, a.k_norm.weight.data, a.k_norm.eps)
        q, k = rope(q, cos, sin).view(B, S, Hq, D), rope(k, cos, sin).view(B, S, Hkv, D)
        rep = Hq // Hkv
        kk, vv = k.repeat_interleave(rep, dim=2), v.repeat_interleave(rep, dim=2)
        sc = torch.einsum("bqhd,bkhd->bhqk", q, kk) * D ** -0.5
        p = torch.softmax(sc.masked_fill(~causal, float("-inf")), dim=-1)
        o = torch.einsum("bhqk,bkhd->bqhd", p, vv).reshape(B * S, Hq * D)
        x = qdq(o) @ qdq(a.o_proj.weight.data).t() + x
        h = rmsnorm(x, n2.weight.data, n2.eps)
        u = qdq(h) @ qdq(ml._wgu.tensor()).t()
        if layer.xielu:
            f = ml.act_fn
            act = xielu(u, f.alpha_p.data, f.alpha_n.data, float(f.beta), float(f.eps))
        else:
            act = torch.nn.functional.silu(u[:, : ml.I]) * u[:, ml.I:]
        x = qdq(act) @ qdq(ml.down_proj.weight.data).t() + x
    x = rmsnorm(x, m.model.norm.weight.data, m.model.norm.eps)
    return (x @ m.lm_head.weight.data.double().t()).view(B, S, -1)
