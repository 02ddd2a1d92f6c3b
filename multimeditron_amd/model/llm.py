"""Llama / Qwen2 / Qwen3 / Apertus decoder on libmmhip kernels: the MI355X replacement for the HF `AutoModelForCausalLM` the
reference constructs at model.py:253-260 and calls at model.py:517-526 (forward) and :595-602 (decode).

Semantics follow HF transformers 5.15.0 (models/llama/modeling_llama.py): RMSNorm :53-70, RoPE :113-160 (+ llama3
inv_freq scaling modeling_rope_utils.py:641-662), GQA softmax attention :191-281, SwiGLU MLP :163-176, pre-norm
residual layer :284-325, final norm + lm_head :413,480, shifted CE loss/loss_utils.py:36-71.  Qwen2 = same graph with
biased q/k/v projections.  Qwen3 = Llama with a per-head RMSNorm of q and k (`q_norm` / `k_norm`, weights [head_dim]) between
the projection and RoPE (HF 5.15 models/qwen3/modeling_qwen3.py:50-64,237-257).  Apertus (HF 5.15 models/apertus/modeling_apertus.py) =
Llama with that q/k norm, llama3 RoPE, the layer norms named `attention_layernorm` / `feedforward_layernorm`, and an ungated MLP
`down_proj(xIELU(up_proj(x)))` whose activation carries two trainable scalars per layer (csrc/mm_xielu.hip).  Parameter names equal
HF's so reference checkpoints interchange.

Data layout: activations are [B*S, features] row-major in HBM; q/k/v come out of ONE fused GEMM as a
[B*S, (Hq+2Hkv)*D] buffer that RoPE rewrites in place and the attention kernel reads through strides; gate/up come
out of one fused GEMM as [B*S, 2I]; the residual add is the GEMM epilogue of o_proj/down_proj."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from functools import partial
from typing import Any, Dict, List, NamedTuple, Optional

import torch
import torch.nn as nn

from .. import functional as Fm
from .. import kernels as K
from ..nn import Embedding, Linear, Norm, grad_dummy


@dataclass
class LLMConfig:
    model_type: str = "llama"
    hidden_size: int = 4096
    intermediate_size: int = 14336
    num_hidden_layers: int = 32
    num_attention_heads: int = 32
    num_key_value_heads: int = 8
    head_dim: Optional[int] = None
    vocab_size: int = 128256
    rms_norm_eps: float = 1e-5
    tie_word_embeddings: bool = False
    attention_bias: bool = False
    qk_norm: bool = False              # Qwen3, Apertus: RMSNorm over every q and k head before RoPE
    hidden_act: str = "silu"           # "silu": gated SwiGLU MLP; "xielu" (Apertus): down_proj(xIELU(up_proj(x)))
    pad_token_id: Optional[int] = None # Apertus (ApertusConfig's default 3): embed_tokens' padding_idx, whose row gets no gradient
    max_position_embeddings: int = 131072
    rope_parameters: Dict[str, Any] = field(default_factory=lambda: {"rope_type": "default", "rope_theta": 10000.0})

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "LLMConfig":
        d = dict(d)
        rp = d.get("rope_parameters")
        if not rp:   # older HF layout: rope_theta + rope_scaling
            rp = dict(d.get("rope_scaling") or {})
            rp.setdefault("rope_type", rp.pop("type", "default"))
            rp.setdefault("rope_theta", d.get("rope_theta", 10000.0))
        mt = d.get("model_type", "llama")
        known = {f for f in cls.__dataclass_fields__}
        kw = {k: v for k, v in d.items() if k in known}
        kw["rope_parameters"] = rp
        if mt.startswith("qwen2"):
            kw["attention_bias"] = True          # Qwen2 hard-codes biased q/k/v (HF:models/qwen2)
        if mt.startswith("qwen3"):
            if mt != "qwen3":
                raise NotImplementedError(f"model_type {mt!r}: only dense Qwen3 decoders are supported")
            if "sliding_attention" in (d.get("layer_types") or ()):
                raise NotImplementedError("Qwen3 sliding-window attention layers are not supported")
            kw["qk_norm"] = True                 # Qwen3: q_norm / k_norm per head (HF:models/qwen3:237-257)
        if mt == "apertus":                      # HF 5.15 models/apertus: q/k norm as Qwen3, an ungated xIELU MLP, its own norm names
            act = d.get("hidden_act", "xielu")
            if act != "xielu":
                raise NotImplementedError(f"Apertus with hidden_act {act!r}: only the xIELU MLP is supported")
            kw["qk_norm"] = True
            kw["hidden_act"] = "xielu"
            kw["pad_token_id"] = d.get("pad_token_id", 3)
        else:
            kw["hidden_act"] = "silu"            # every other family here is the gated SiLU MLP, whatever the field says
            kw["pad_token_id"] = None            # ... and keeps its embedding without a padding row, as before
        if not kw.get("head_dim"):
            kw["head_dim"] = kw.get("hidden_size", 4096) // kw.get("num_attention_heads", 32)
        return cls(**kw)

    def to_dict(self):
        d = {k: getattr(self, k) for k in self.__dataclass_fields__}
        if d["hidden_act"] == "silu":            # written only when it says something: Llama / Qwen configs stay byte-identical
            del d["hidden_act"]
        if d["pad_token_id"] is None:
            del d["pad_token_id"]
        return d

    @property
    def apertus(self) -> bool:
        return self.model_type == "apertus"


def rope_inv_freq(cfg: LLMConfig) -> torch.Tensor:
    rp = cfg.rope_parameters
    base = float(rp.get("rope_theta", 10000.0))
    hd = cfg.head_dim
    inv = 1.0 / (base ** (torch.arange(0, hd, 2, dtype=torch.int64).to(torch.float32) / hd))
    if rp.get("rope_type", "default") == "llama3":
        factor, lo, hi = rp["factor"], rp["low_freq_factor"], rp["high_freq_factor"]
        old = rp["original_max_position_embeddings"]
        wavelen = 2 * math.pi / inv
        scaled = torch.where(wavelen > old / lo, inv / factor, inv)
        smooth = (old / wavelen - lo) / (hi - lo)
        mid = (1 - smooth) * scaled / factor + smooth * scaled
        is_mid = ~(wavelen < old / hi) * ~(wavelen > old / lo)
        inv = torch.where(is_mid, mid, scaled)
    return inv


class Attention(nn.Module):
    def __init__(self, cfg: LLMConfig, dtype, device):
        super().__init__()
        H, D = cfg.hidden_size, cfg.head_dim
        self.Hq, self.Hkv, self.D = cfg.num_attention_heads, cfg.num_key_value_heads, D
        b = cfg.attention_bias
        self.q_proj = Linear(H, self.Hq * D, bias=b, dtype=dtype, device=device)
        self.k_proj = Linear(H, self.Hkv * D, bias=b, dtype=dtype, device=device)
        self.v_proj = Linear(H, self.Hkv * D, bias=b, dtype=dtype, device=device)
        self.o_proj = Linear(self.Hq * D, H, bias=False, dtype=dtype, device=device)
        self._wqkv = Fm.ParamGroup([self.q_proj.weight, self.k_proj.weight, self.v_proj.weight])
        self._bqkv = Fm.ParamGroup([self.q_proj.bias, self.k_proj.bias, self.v_proj.bias]) if b else None
        self.q_norm = Norm(D, cfg.rms_norm_eps, bias=False, dtype=dtype, device=device) if cfg.qk_norm else None
        self.k_norm = Norm(D, cfg.rms_norm_eps, bias=False, dtype=dtype, device=device) if cfg.qk_norm else None

    def qkn(self):
        """(q_norm weight, k_norm weight, eps) of a Qwen3 layer, else None."""
        return None if self.q_norm is None else (self.q_norm.weight, self.k_norm.weight, self.q_norm.eps)

    def rope_views(self, qkv, cos, sin, B, S):
        """(per-head norm +) RoPE of the fused projection in place (no autograd: nothing keeps a backward) -> its q, k, v as strided
        views."""
        Hq, Hkv, D = self.Hq, self.Hkv, self.D
        if self.q_norm is not None:
            K.qk_norm_rope_fwd(qkv, B * S, Hq, Hkv, D, *self.qkn(), cos, sin, out=qkv, want_rstd=False)
        else:
            K.rope_apply_(qkv, B * S, Hq + Hkv, D, (Hq + 2 * Hkv) * D, cos, sin)
        return Fm.qkv_views(qkv, B, S, Hq, Hkv, D)

    def rope_append_(self, qkv, B, cos, sin, kcache, vcache, pos):
        """A decode step's (per-head norm +) RoPE of q / k in place and the write of the new k / v rows to cache[:, pos]: one pass."""
        if self.q_norm is not None:
            K.qk_norm_rope_append_(qkv, B, self.Hq, self.Hkv, self.D, *self.qkn(), cos, sin, kcache, vcache, pos)
        else:
            K.rope_append_(qkv, B, self.Hq, self.Hkv, self.D, cos, sin, kcache, vcache, pos)


class MLP(nn.Module):
    def __init__(self, cfg: LLMConfig, dtype, device):
        super().__init__()
        H, I = cfg.hidden_size, cfg.intermediate_size
        self.I = I
        self.gate_proj = Linear(H, I, bias=False, dtype=dtype, device=device)
        self.up_proj = Linear(H, I, bias=False, dtype=dtype, device=device)
        self.down_proj = Linear(I, H, bias=False, dtype=dtype, device=device)
        self._wgu = Fm.ParamGroup([self.gate_proj.weight, self.up_proj.weight])


class XIELU(nn.Module):
    """Holder of HF's XIELUActivation state (activations.py, transformers 5.15): the raw scalars `alpha_p`, `alpha_n` (Parameters of
    shape [1], model dtype; the kernels apply the softplus) and the persistent 0-dim buffers `beta`, `eps` (model dtype, so a bf16
    model carries eps = bf16(-1e-6), which is what its arithmetic uses)."""

    def __init__(self, dtype, device, alpha_p_init=0.8, alpha_n_init=0.8, beta=0.5, eps=-1e-6):
        super().__init__()
        self.alpha_p = nn.Parameter(torch.log(torch.expm1(torch.tensor(alpha_p_init, dtype=dtype))).unsqueeze(0).to(device))
        self.alpha_n = nn.Parameter(torch.log(torch.expm1(torch.tensor(alpha_n_init - beta, dtype=dtype))).unsqueeze(0).to(device))
        self.register_buffer("beta", torch.tensor(beta, dtype=dtype, device=device))
        self.register_buffer("eps", torch.tensor(eps, dtype=dtype, device=device))
        self._consts = None

    def consts(self):
        """(beta, eps) as floats for the kernels' arguments: read from the buffers once per value (a host read), not per call."""
        key = (self.beta._version, self.eps._version, self.beta.data_ptr(), self.eps.data_ptr())
        if self._consts is None or self._consts[0] != key:
            self._consts = (key, (float(self.beta), float(self.eps)))
        return self._consts[1]


class XIELUMLP(nn.Module):
    """Apertus: down_proj(xIELU(up_proj(x))), no gate (HF 5.15 models/apertus/modeling_apertus.py ApertusMLP)."""

    def __init__(self, cfg: LLMConfig, dtype, device):
        super().__init__()
        H, I = cfg.hidden_size, cfg.intermediate_size
        self.I = I
        self.up_proj = Linear(H, I, bias=False, dtype=dtype, device=device)
        self.down_proj = Linear(I, H, bias=False, dtype=dtype, device=device)
        self.act_fn = XIELU(dtype, device)
        self._wgu = Fm.ParamGroup([self.up_proj.weight])      # the MLP's first GEMM operand, under the name the gated MLP uses

    def act(self, u):
        """xIELU of the pre-activation (no autograd: prefill and decode)."""
        f = self.act_fn
        return K.xielu_fwd(u, f.alpha_p.data, f.alpha_n.data, *f.consts())


class W16(NamedTuple):
    """One matrix of the inference chains in the model's own format (a layer's fused q|k|v, o_proj, fused gate|up / up_proj,
    down_proj, or lm_head): the launches that read it.  Holds where to read the tensor, not the tensor: packing, .to() and
    resize_token_embeddings move it.  The chains queue these launches once per layer and token: plain positional calls."""
    get: Any      # () -> the weight: a ParamGroup's tensor, or partial(getattr, linear, "weight")

    def linear(self, x, mx8=False, **kw):
        """mm_gemm (which streams the weights itself when x has at most 16 rows)."""
        assert not mx8
        return K.linear_fwd(x, self.get(), **kw)

    def stream(self, x, residual=None, norm_w=None, eps=0.0, ldc_pad=False):
        """The weight-streaming linear of a decode step, with its optional fused RMSNorm (norm_w, eps), residual and ldc_pad."""
        return K.decode_linear(x, self.get(), None, residual, norm_w, eps, ldc_pad)

    def qkv_rope_append(self, x, bias, Hq, Hkv, D, cos, sin, kcache, vcache, pos, norm_w, eps):
        return K.decode_qkv_rope_append(x, self.get(), bias, Hq, Hkv, D, cos, sin, kcache, vcache, pos, norm_w, eps)

    def gateup_swiglu(self, x, I, norm_w, eps):
        return K.decode_gateup_swiglu(x, self.get(), I, norm_w, eps)


class W8(NamedTuple):
    """The same matrix as its MXFP8 copy (CausalLM.quantize_decode_weights): the packed buffer and the number of output features."""
    packed: torch.Tensor
    N: int

    def linear(self, x, mx8=False, **kw):
        """Weight-only (a decode step: the bf16 x streams the copy), or mx8=True the prefill's MXFP8 x MXFP8 GEMM on the
        block-scaled MFMA: x quantised at the rounding point where the bf16 chain hands it to its GEMM."""
        if mx8:
            return K.gemm_mx8(K.quant_mxfp8(x), x.shape[0], self.packed, self.N, x.shape[1], **kw)
        return K.decode_linear_w8(x, self.packed, self.N, **kw)

    def stream(self, x, residual=None, norm_w=None, eps=0.0, ldc_pad=False):
        return K.decode_linear_w8(x, self.packed, self.N, None, residual, norm_w, eps, ldc_pad)

    def qkv_rope_append(self, x, bias, Hq, Hkv, D, cos, sin, kcache, vcache, pos, norm_w, eps):
        return K.decode_qkv_rope_append_w8(x, self.packed, bias, Hq, Hkv, D, cos, sin, kcache, vcache, pos, norm_w, eps)

    def gateup_swiglu(self, x, I, norm_w, eps):
        return K.decode_gateup_swiglu_w8(x, self.packed, I, norm_w, eps)


class Plan(NamedTuple):
    """How a call without autograd runs its layers: CausalLM.forward decides it once per call, DecoderLayer.infer picks the form of
    every stage from it."""
    rows: str       # "step": at most 16 bf16 rows over a filled cache (one new token per sequence, or the k + 1 positions of a
                    # prompt-lookup verify step), every linear one weight-streaming launch; "prefill": the MXFP8 prefill
    fused: bool     # a step whose norms and SwiGLU ride in the weight-streaming launches (can_decode_step_fused / can_verify_fused)


class DecoderLayer(nn.Module):
    def __init__(self, cfg: LLMConfig, dtype, device):
        super().__init__()
        self.self_attn = Attention(cfg, dtype, device)
        self.xielu = cfg.hidden_act == "xielu"
        self.mlp = XIELUMLP(cfg, dtype, device) if self.xielu else MLP(cfg, dtype, device)
        n1, n2 = ("attention_layernorm", "feedforward_layernorm") if cfg.apertus else ("input_layernorm", "post_attention_layernorm")
        setattr(self, n1, Norm(cfg.hidden_size, cfg.rms_norm_eps, bias=False, dtype=dtype, device=device))
        setattr(self, n2, Norm(cfg.hidden_size, cfg.rms_norm_eps, bias=False, dtype=dtype, device=device))
        self._norm_names = (n1, n2)
        a, m = self.self_attn, self.mlp
        self.w16 = {"qkv": W16(a._wqkv.tensor), "o": W16(partial(getattr, a.o_proj, "weight")), "gu": W16(m._wgu.tensor),
                    "down": W16(partial(getattr, m.down_proj, "weight"))}

    def norms(self):
        """(the norm in front of attention, the norm in front of the MLP): HF names them differently for Apertus."""
        return getattr(self, self._norm_names[0]), getattr(self, self._norm_names[1])

    @torch.no_grad()
    def infer(self, w, x, cos, sin, key_mask, B, S, cache, plan: Plan):
        """The layer without autograd, on the matrices w (this layer's W16s, or its W8s from CausalLM.quantize_decode_weights -- the
        same launches on half the weight bytes): q|k|v -> attend -> o_proj + residual -> gate|up (Apertus: up_proj) + activation ->
        down_proj + residual, with the arithmetic and rounding points of forward() in every form.  x = residual stream in and out.

        plan.rows == "step": M = B S <= 16 rows over a filled cache -- a decode step (S = 1, generate's loop, reference
        model.py:595-602) or a prompt-lookup verify step (S = k + 1 positions per sequence) --, so every linear is one
        weight-streaming launch that reads its matrix once (W16: mm_gemm's M <= 16 kernel; W8: the weight-only kernel), and the cache
        places and attends the new rows (its `step`).  plan.fused folds the tiny launches into those (csrc/mm_gemm.hip
        gemv_stream_kernel): a decode step is 6 launches with the two attention kernels, none of them a norm, and has the bits of
        the separate form.
        plan.rows == "prefill": the MXFP8 prefill (forward(prefill_weights="mxfp8"), w = the W8s).  Each linear is quant_mxfp8 of its
        bf16 input + gemm_mx8; everything but those eight launches is the existing kernel on bf16 data."""
        a, m = self.self_attn, self.mlp
        Hq, Hkv, D = a.Hq, a.Hkv, a.D
        n1, n2 = self.norms()
        step = plan.rows == "step"
        mx8 = not step
        bias = a._bqkv.tensor() if a._bqkv is not None else None
        # q|k|v.  fused: input RMSNorm + q|k|v + RoPE + cache append in one launch where the cache knows on the host where the new
        # row goes, else input RMSNorm + q|k|v where there is no bias (the plain streaming linear carries none: a fused verify
        # step, can_verify_fused) and the cache ropes and places the rows itself.  separate:
        # folding RMSNorm / SwiGLU into the GEMM's own x operand was measured SLOWER (every workgroup redoes the transform on all 64
        # lanes and the kernel turns VALU-bound, 43 vs 27 us and 57 vs 25 us per launch), so they are launches of their own
        dst = cache.append_dst() if plan.fused else None
        if dst is not None:
            qkv = w["qkv"].qkv_rope_append(x, bias, Hq, Hkv, D, cos, sin, *dst, n1.weight, n1.eps)
        elif plan.fused and bias is None:
            qkv = w["qkv"].stream(x, None, n1.weight, n1.eps)
        else:
            h, _ = K.rmsnorm_fwd(x, n1.weight, n1.eps)
            qkv = w["qkv"].linear(h, mx8, bias=bias)
        # attend: RoPE / q-k norm, the cache append and the attention kernel are the cache's; without a cache rope_views + attn_fwd
        if step:
            o = cache.step(qkv, cos, sin, key_mask, B, S, a, dst is not None)
        elif cache is not None:
            o = cache.attend(qkv, cos, sin, key_mask, B, S, a)
        else:
            q, kn, vn = a.rope_views(qkv, cos, sin, B, S)
            o = K.attn_fwd(q, kn, vn, key_mask, True, D ** -0.5)[0].view(B * S, Hq * D)
        # tail.  fused: o_proj + residual, post-attention RMSNorm + gate|up + SwiGLU, down_proj + residual -- down_proj in the
        # LDS-staged launch where its M rows of I features fit it, else in mm_gemm's M <= 16 kernel (the same bits): 16 rows of the
        # 8B model's 14336 features do not fit, its 4096-wide inputs do; a decode step always fits (can_decode_step_fused)
        if plan.fused:
            x = w["o"].stream(o, x)
            act = w["gu"].gateup_swiglu(x, m.I, n2.weight, n2.eps)
            return w["down"].stream(act, x) if K.decode_fits(B * S, m.I) else w["down"].linear(act, residual=x)
        x = w["o"].linear(o, mx8, residual=x)
        h, _ = K.rmsnorm_fwd(x, n2.weight, n2.eps)
        u = w["gu"].linear(h, mx8)
        act = m.act(u) if self.xielu else K.swiglu_fwd(u, m.I)
        return w["down"].linear(act, mx8, residual=x)

    def can_decode_step(self, x, B, S, cache):
        a = self.self_attn
        return (cache is not None and S == 1 and B <= 16 and x.dtype == torch.bfloat16 and not torch.is_grad_enabled()
                and K.attn_decode_supported(x.dtype, a.Hq, a.Hkv, a.D))

    def _can_fuse(self, x, M):
        """What folding the norms and SwiGLU into the weight-streaming launches asks of the layer and of M rows, whatever the step."""
        a = self.self_attn
        return (a.D == 128 and a.q_norm is None and K.decode_fusions() and x.shape[-1] <= 8192 and self.mlp.I % 4 == 0
                and K.decode_fits(M, x.shape[-1]) and K.decode_fits(M, a.Hq * a.D)
                and a.o_proj.bias is None and self.mlp.down_proj.bias is None and self.norms()[0].bias is None)

    def can_decode_step_fused(self, x, B, S, cache):
        """... of a decode step: down_proj's B input rows fit the LDS stage as well."""
        return self.can_decode_step(x, B, S, cache) and self._can_fuse(x, B) and K.decode_fits(B, self.mlp.I)

    def can_verify_fused(self, x, M):
        """... of a verify step of M = B (k + 1) rows: no q|k|v bias (the plain streaming linear carries none here) and, by name,
        no xIELU; infer places down_proj by itself."""
        return self._can_fuse(x, M) and self.self_attn._bqkv is None and not self.xielu

    def forward(self, x, cos, sin, key_mask, B, S, cache=None, rows=None):
        """The training / generic route (CausalLM.forward has decided that the call is neither a decode step nor an MXFP8 prefill).
        rows (functional.LossRows, LAST layer of a training forward only): nothing after this layer's attention reads the
        rows that carry no label -- their hidden states feed no later layer and no loss term -- so o_proj, the post-attention norm
        and the MLP run on the labelled rows alone and the layer returns [rows.n, H].  (Keys and values come from every row, so
        attention itself is computed in full.)  Same loss, same gradients."""
        a = self.self_attn
        n1, n2 = self.norms()
        h, x = n1(x)
        if cache is None:      # projection (+ RoPE in its epilogue) + attention as one autograd node
            o = Fm.qkv_rope_attention(h, a._wqkv, a._bqkv, cos, sin, key_mask, B, S, a.Hq, a.Hkv, a.D, True, a.D ** -0.5,
                                      dummy=grad_dummy(a.q_proj.weight), qkn=a.qkn())
        else:
            qkv = Fm.linear(h, a._wqkv, a._bqkv, dummy=grad_dummy(a.q_proj.weight))
            o = cache.attend(qkv, cos, sin, key_mask, B, S, a)
        if rows is not None:
            o, x = Fm.rows_select(o, rows), Fm.rows_select(x, rows)
        x = a.o_proj(o, residual=x)
        h, x = n2(x)
        if self.xielu:
            m = self.mlp
            return Fm.xielu_mlp(h, m._wgu, m.down_proj.weight, m.act_fn, residual=x, dummy=grad_dummy(m.up_proj.weight))
        return Fm.swiglu_mlp(h, self.mlp._wgu, self.mlp.down_proj.weight, self.mlp.I, residual=x,
                             dummy=grad_dummy(self.mlp.gate_proj.weight))


class LayerKVCache:
    """Contiguous per-layer KV cache [B, Smax, Hkv, D] for the decode loop of generate (model.py:581-638).  A cache answers three
    things: how many positions it holds (positions), the attention of S new positions from an unroped fused projection (attend: the
    prefill, and the steps of the generic route) and the attention of a decode or verify step (step).  A subclass changes where the
    rows are kept and which decode attention reads them."""

    stream_only = False      # whether ONE new position can be attended by the decode stream alone (else: where attn_decode takes it)
    staged = False           # whether append_dst() is a staging row that store() moves into place

    def __init__(self, B, Smax, Hkv, D, dtype, device):
        self.k = torch.zeros((B, Smax, Hkv, D), dtype=dtype, device=device)
        self.v = torch.zeros((B, Smax, Hkv, D), dtype=dtype, device=device)
        self.len = 0

    def positions(self):
        """How many positions of every sequence the cache holds: where the next one goes."""
        return self.len

    def append_dst(self):
        """(kcache, vcache, pos) of a decode step's append kernels: where the new token's k / v rows go.  None from a cache that
        does not know the position on the host."""
        return self.k, self.v, self.len

    def accept(self, B, S):
        """ValueError for a call of S new positions on B rows that this cache does not take."""

    def store(self, kn, vn, S):
        """The S new k / v rows go behind the `len` held ones (device-side memory plumbing) -> the keys and values attn_fwd reads
        once they are counted."""
        self.k[:, self.len:self.len + S].copy_(kn)
        self.v[:, self.len:self.len + S].copy_(vn)
        return self.k[:, : self.len + S], self.v[:, : self.len + S]

    def decode_attend(self, q, key_mask, scale):
        """The row of position `len` has been written and nothing has attended over it yet: count it and attend q [B, Hq, D] over
        the cache (split-K stream)."""
        self.len += 1
        return K.attn_decode(q, self.k[:, : self.len], self.v[:, : self.len], key_mask, scale)

    @torch.no_grad()
    def attend(self, qkv, cos, sin, key_mask, B, S, a: Attention):
        """The fused projection of S new positions -> their attention output [B S, Hq D]: check what this cache accepts, RoPE,
        store the new rows, attend over them."""
        Hq, D = a.Hq, a.D
        self.accept(B, S)
        q, kn, vn = a.rope_views(qkv, cos, sin, B, S)
        kv = self.store(kn, vn, S)
        if S == 1 and (self.stream_only or K.attn_decode_supported(qkv.dtype, Hq, a.Hkv, D)):      # stream the cache once (split-K)
            return self.decode_attend(q.view(B, Hq, D), key_mask, D ** -0.5).view(B, Hq * D)
        self.len += S
        return K.attn_fwd(q, *kv, key_mask, True, D ** -0.5)[0].view(B * S, Hq * D)

    def step(self, qkv, cos, sin, key_mask, B, S, a: Attention, appended):
        """The fused projection of a decode step (S = 1; B <= 16 bf16 rows) -> its attention output [B, Hq D].  appended: the
        projection's launch has roped q / k and written the new rows to append_dst() already; else that is one pass here
        (rope_append_ / qk_norm_rope_append_)."""
        if not appended:
            a.rope_append_(qkv, B, cos, sin, *self.append_dst())
        if self.staged:
            self.store(self.k, self.v, 1)
        return self.decode_attend(qkv[:, : a.Hq * a.D].view(B, a.Hq, a.D), key_mask, a.D ** -0.5).view(B, a.Hq * a.D)


class LayerKVCacheMX8(LayerKVCache):
    """The same cache in MXFP8 (include/mm_hip.h: mm_kv8_*): ONE uint8 buffer of mm_kv8_bytes for K and V, elements and scales
    (1 + 1/32 byte per element, 0.516 of bf16; the layout is the library's), and a bf16 staging row [B, 1, Hkv, D] each for k and v.
    A decode step's append kernels write the new row to the staging row (position 0) unchanged; mm_kv8_append quantises it into
    position `len` and mm_attn_decode_kv8 streams the buffer.  The prefill attends over the bf16 k / v of the prompt (its output is
    the bf16 cache's, bit for bit) and quantises them into the buffer in one pass; only later steps see quantised keys."""

    stream_only = True
    staged = True

    def __init__(self, B, Smax, Hkv, D, dtype, device):
        self.Smax, self.Hkv = Smax, Hkv
        self.buf = torch.zeros((K.kv8_bytes(B, Smax, Hkv, D),), dtype=torch.uint8, device=device)
        self.k = torch.zeros((B, 1, Hkv, D), dtype=dtype, device=device)
        self.v = torch.zeros((B, 1, Hkv, D), dtype=dtype, device=device)
        self.len = 0

    def append_dst(self):
        return self.k, self.v, 0

    def accept(self, B, S):
        if S > 1 and self.len:
            raise ValueError(f"{S} new positions on an MXFP8 KV cache that holds {self.len}: only a prefill into an empty cache or "
                             "one token per step (attending over the cached prompt would need a dequantising prefill)")

    def store(self, kn, vn, S):
        K.kv8_append(kn, vn, self.buf, self.Smax, self.len)
        return kn, vn      # a prefill's cache was empty: the prompt's own bf16 rows

    def decode_attend(self, q, key_mask, scale):
        self.len += 1
        return K.attn_decode_kv8(q, self.buf, self.len, self.Smax, self.Hkv, key_mask, scale)


class LayerKVCacheShared(LayerKVCache):
    """The cache of generate(num_return_sequences=n): the prompt's keys and values ONCE per prompt, k / v [B, Sp_max, Hkv, D] (`len`
    positions filled), and the tokens each of the B n sample rows has generated in ks / vs [B n, max_new, Hkv, D] (`slen` filled).
    Row r = b n + j is sample j of prompt b and attends over [prefix of b | suffix of r] (include/mm_hip.h: mm_attn_decode_shared;
    the bits of a LayerKVCache of B n rows that holds the prompt n times).  The prefill is a call of B rows into the empty cache
    (the base class's steps: it writes the prefix); every later call brings ONE token for each of the B n rows, and its key_mask is
    the PROMPT's [B, len] (suffix keys are always visible)."""

    stream_only = True
    kind = "a shared-prefix cache"

    def __init__(self, B, n, Sp_max, max_new, Hkv, D, dtype, device):
        super().__init__(B, Sp_max, Hkv, D, dtype, device)
        self.B, self.n = B, n
        self.ks = torch.zeros((B * n, max(1, max_new), Hkv, D), dtype=dtype, device=device)
        self.vs = torch.zeros((B * n, max(1, max_new), Hkv, D), dtype=dtype, device=device)
        self.slen = 0

    def positions(self):
        return self.len + self.slen

    def append_dst(self):
        """(suffix k, suffix v, slen): the append kernels write row r's new key / value at its own suffix position."""
        if self.slen >= self.ks.shape[1]:
            raise ValueError(f"the shared-prefix KV cache is full: {self.slen} generated tokens per sample row")
        return self.ks, self.vs, self.slen

    def ancestors(self):
        """The table through which the suffix keys are read: None, every row reads its own."""
        return None

    def decode_attend(self, q, key_mask, scale):
        """The suffix row of position `slen` has been written for every sample: count it and attend q [B n, Hq, D]."""
        if key_mask is not None and tuple(key_mask.shape) != (self.B, self.len):
            raise ValueError(f"key_mask of shape {tuple(key_mask.shape)} on {self.kind}: the prompt's mask [{self.B}, {self.len}] is "
                             "expected (generated tokens are always visible)")
        anc = self.ancestors()
        self.slen += 1
        return K.attn_decode_shared(q, self.k[:, : self.len], self.v[:, : self.len], self.ks[:, : self.slen], self.vs[:, : self.slen],
                                    self.n, key_mask, scale, anc)

    def accept(self, B, S):
        if S > 1 and (self.len or B != self.B):
            raise ValueError(f"{S} new positions for {B} rows on a shared-prefix KV cache of {self.B} prompts that holds {self.len}: only "
                             "a prefill of the prompts into an empty cache or one token per sample row")
        if S == 1 and (B != self.B * self.n or not self.len):
            raise ValueError(f"a step of {B} rows on a shared-prefix KV cache of {self.B} x {self.n} sample rows that holds {self.len} "
                             "prompt positions")
        if S == 1:
            self.append_dst()      # raises when the suffix is full

    def store(self, kn, vn, S):
        if S > 1:
            return super().store(kn, vn, S)          # the prefill on B rows: writes the prefix
        ks, vs, pos = self.append_dst()
        ks[:, pos:pos + 1].copy_(kn)      # device-side memory plumbing
        vs[:, pos:pos + 1].copy_(vn)


class LayerKVCacheBeam(LayerKVCacheShared):
    """The cache of generate(num_beams=n): LayerKVCacheShared whose suffix is read through an ancestor table.  Row r still WRITES
    its new key / value into its own suffix row, but suffix key t of row r is READ from physical row table[t, r] (include/mm_hip.h:
    mm_attn_decode_beam), so a beam that continues another row's hypothesis costs a column of int32 instead of HF's reorder_cache
    (an index_select over every layer's whole cache).  All layers share ONE table holder: the decode loop sets `tables.current` to
    the table mm_beam_step wrote for the coming step (K.BeamState.table) before it calls the decoder."""

    kind = "a beam cache"

    class Tables:
        current = None           # int32 [>= slen, >= B n]

    def __init__(self, B, n, Sp_max, max_new, Hkv, D, dtype, device, tables):
        super().__init__(B, n, Sp_max, max_new, Hkv, D, dtype, device)
        self.tables = tables

    def ancestors(self):
        anc = self.tables.current
        if anc is None or anc.shape[0] <= self.slen:
            raise ValueError(f"a step on a beam KV cache without an ancestor table of more than {self.slen} rows")
        return anc


class LayerKVCacheGuided(LayerKVCache):
    """The cache of generate(guidance_scale=): ONE plain LayerKVCache of 2 B rows for the B conditional sequences (rows [0, B)) and
    their B unconditional partners (rows [B, 2 B)), whose prompts have different padded lengths Sc and Su.  It has Sp = max(Sc, Su)
    prompt slots and room for max_new generated tokens, and takes exactly: a prefill of B rows x Sc into the empty cache (slots
    [Sp - Sc, Sp) of rows [0, B)), then a prefill of B rows x Su (slots [Sp - Su, Sp) of rows [B, 2 B)), then steps of 2 B rows x 1.
    Each prefill attends over its own rows alone, at its own length -- what a LayerKVCache of B rows would compute --; placing the
    rows is device-side plumbing.  Both halves end at slot Sp, so a step is an ordinary left-padded batch of 2 B rows over Sp + i
    keys (the base class's append and decode attention, the fused step included) under a key_mask [2 B, Sp + i] that is 0 on the
    slots in front of the shorter half (they hold zeros).  positions() is 0 until both prefills are in: to CausalLM.forward either
    one is a prefill into an empty cache."""

    def __init__(self, B, Sp_max, max_new, Hkv, D, dtype, device):
        super().__init__(2 * B, Sp_max + max(1, max_new), Hkv, D, dtype, device)
        self.B, self.Sp, self.prefills = B, Sp_max, 0

    def positions(self):
        return self.len if self.prefills == 2 else 0

    def append_dst(self):
        """The base class's once both prefills are in.  None before: a one-token prompt's prefill is a decode step that `step`
        places itself, after `accept` has seen its rows."""
        return super().append_dst() if self.prefills == 2 else None

    def accept(self, B, S):
        if self.prefills < 2 and (B != self.B or not 1 <= S <= self.Sp):
            raise ValueError(f"{S} new positions for {B} rows on a guided KV cache of {self.B} pairs and {self.Sp} prompt slots that holds "
                             f"{self.prefills} of its two prefills: only the conditional prefill, then the unconditional one, each of "
                             f"{self.B} rows and at most {self.Sp} positions, then one token per row of both halves")
        if self.prefills == 2 and (B != 2 * self.B or S != 1 or self.len >= self.k.shape[1]):
            raise ValueError(f"{S} new positions for {B} rows on a guided KV cache of {self.B} pairs that holds both prefills and "
                             f"{self.len} of {self.k.shape[1]} positions: only one token for each of its {2 * self.B} rows")

    def _half(self, S):
        """(k, v, first slot) of the half the coming prefill of S positions fills."""
        rows = slice(self.prefills * self.B, (self.prefills + 1) * self.B)
        return self.k[rows], self.v[rows], self.Sp - S

    def _filled(self):
        self.prefills += 1
        if self.prefills == 2:
            self.len = self.Sp

    @torch.no_grad()
    def attend(self, qkv, cos, sin, key_mask, B, S, a: Attention):
        if self.prefills == 2:
            return super().attend(qkv, cos, sin, key_mask, B, S, a)
        Hq, D = a.Hq, a.D
        self.accept(B, S)
        q, kn, vn = a.rope_views(qkv, cos, sin, B, S)
        k, v, at = self._half(S)
        k[:, at:at + S].copy_(kn)      # device-side memory plumbing
        v[:, at:at + S].copy_(vn)
        self._filled()
        if S == 1 and K.attn_decode_supported(qkv.dtype, Hq, a.Hkv, D):
            return K.attn_decode(q.view(B, Hq, D), k[:, at:at + S], v[:, at:at + S], key_mask, D ** -0.5).view(B, Hq * D)
        return K.attn_fwd(q, k[:, at:at + S], v[:, at:at + S], key_mask, True, D ** -0.5)[0].view(B * S, Hq * D)

    def step(self, qkv, cos, sin, key_mask, B, S, a: Attention, appended):
        self.accept(B, S)
        if self.prefills == 2:
            return super().step(qkv, cos, sin, key_mask, B, S, a, appended)
        k, v, at = self._half(1)       # a one-token prompt (HF's default unconditional prompt): a decode step over its own key
        a.rope_append_(qkv, B, cos, sin, k, v, at)
        self._filled()
        return K.attn_decode(qkv[:, : a.Hq * a.D].view(B, a.Hq, a.D), k[:, at:at + 1], v[:, at:at + 1], key_mask, a.D ** -0.5).view(B, a.Hq * a.D)


class LayerKVCacheLookup(LayerKVCache):
    """The cache of generate(prompt_lookup_num_tokens=k): a bf16 LayerKVCache [B, Smax, Hkv, D] whose rows advance by DIFFERENT
    amounts per verify step, so where a row stands is not a host integer: `shared.base` (int32 [B] on the device, advanced by
    mm_lookup_accept) is the position and cache slot of every row's newest id.  The prefill is the base class's (it fills `len`
    positions of every row); a verify step writes its Q = k + 1 new k / v rows at the slots base[b] + j (mm_kv_append_at) and attends
    query (b, j) over the keys t <= base[b] + j (mm_attn_decode_verify).  Slots behind a row's accepted ids hold rejected drafts: no
    query sees them and the next step overwrites them.  All layers share ONE `Shared` object, as LayerKVCacheBeam's layers share their
    tables: the decode loop sets `shared.bound`, a host-side upper bound of every base[b], before it calls the decoder."""

    class Shared:
        base = None              # int32 [B], device
        bound = 0                # base[b] <= bound for every row (known without a sync)

    def __init__(self, B, Smax, Hkv, D, dtype, device, shared):
        super().__init__(B, Smax, Hkv, D, dtype, device)
        self.shared = shared

    def append_dst(self):
        """The empty cache's: every row stands at 0 (a one-token prompt's prefill is an ordinary decode step).  Afterwards None: the
        rows stand at base[b], on the device."""
        return None if self.len else super().append_dst()

    def step(self, qkv, cos, sin, key_mask, B, Q, a: Attention, appended):
        """The unroped fused projection qkv [B Q, (Hq + 2 Hkv) D] of a verify step, Q = k + 1 positions for each of B sequences:
        the in-place RoPE (rope_apply_ / qk_norm_rope_fwd), the append of the Q new k / v rows, the Q-position decode attention
        over one read of the keys -> [B Q, Hq D].  Into the empty cache (Q = 1): the base class's decode step."""
        if not self.len:
            return super().step(qkv, cos, sin, key_mask, B, Q, a, appended)
        Hq, Hkv, D = a.Hq, a.Hkv, a.D
        sh = self.shared
        if sh.base is None:
            raise ValueError("a verify step on a prompt-lookup KV cache without a prefill or without its base positions")
        if key_mask is not None and tuple(key_mask.shape) != (B, self.len):
            raise ValueError(f"key_mask of shape {tuple(key_mask.shape)} on a prompt-lookup cache: the prompt's mask [{B}, {self.len}] is "
                             "expected (generated tokens are visible up to each query's own position)")
        a.rope_views(qkv, cos, sin, B, Q)
        K.lookup_append(qkv, B, Q, Hq, Hkv, D, sh.base, self.k, self.v)
        Scap = min(self.k.shape[1], max(int(sh.bound), self.len) + Q)
        return K.attn_decode_verify(qkv[:, : Hq * D].view(B * Q, Hq, D), self.k[:, :Scap], self.v[:, :Scap], Q, key_mask, sh.base,
                                    D ** -0.5).view(B * Q, Hq * D)


class DecoderModel(nn.Module):
    def __init__(self, cfg: LLMConfig, dtype, device):
        super().__init__()
        self.embed_tokens = Embedding(cfg.vocab_size, cfg.hidden_size, dtype=dtype, device=device, padding_idx=cfg.pad_token_id)
        self.layers = nn.ModuleList([DecoderLayer(cfg, dtype, device) for _ in range(cfg.num_hidden_layers)])
        self.norm = Norm(cfg.hidden_size, cfg.rms_norm_eps, bias=False, dtype=dtype, device=device)


@dataclass
class CausalLMOutput:
    loss: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
    past_key_values: Optional[Any] = None
    hidden_states: Optional[Any] = None
    attentions: Optional[Any] = None

    def __getitem__(self, k):
        return getattr(self, k) if isinstance(k, str) else (self.loss, self.logits, self.past_key_values)[k]


def _int_arg(name, v, lo, hi=None):
    """new_cache's "int in range, not bool" check; -> v"""
    if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
        raise ValueError(f"{name} must be an int {f'>= {lo}' if hi is None else f'in [{lo}, {hi}]'}, got {v!r}")
    return v


# new_cache's modes in the order they are looked at: (argument, its largest value, the arguments it cannot be combined with, the refusal)
_CACHE_MODES = (
    ("lookup", None, ("kv_cache", "samples", "beams"),
     "lookup={lookup} with kv_cache={kv_cache!r}, samples={samples!r}, beams={beams!r}: the prompt-lookup cache is bf16 only, one row per sequence"),
    ("beams", 16, ("kv_cache", "samples"),
     "beams={beams} with kv_cache={kv_cache!r}, samples={samples!r}: the beam cache is bf16 only and its rows are the beams"),
    ("samples", None, ("kv_cache",), "samples={samples} with kv_cache={kv_cache!r}: the shared-prefix cache is bf16 only"),
)


class CausalLM(nn.Module):
    """`self.model` of MultiModalModelForCausalLM (reference attribute name, model.py:253-262)."""

    def __init__(self, cfg: LLMConfig, dtype=torch.bfloat16, device=None):
        super().__init__()
        self.config = cfg
        self.model = DecoderModel(cfg, dtype, device)
        self.lm_head = Linear(cfg.hidden_size, cfg.vocab_size, bias=False, dtype=dtype, device=device)
        if cfg.tie_word_embeddings:
            self.lm_head.weight = self.model.embed_tokens.weight
        self._inv_freq = None
        self._decode_w8 = None      # quantize_decode_weights(): plain tensors beside the modules, neither parameters nor buffers
        self._w16 = {"fmt": None, "layers": [layer.w16 for layer in self.model.layers], "lm_head": W16(partial(getattr, self.lm_head, "weight"))}

    # -- reference surface -------------------------------------------------------------------------
    @property
    def device(self):
        return self.model.embed_tokens.weight.device

    @property
    def dtype(self):
        return self.model.embed_tokens.weight.dtype

    def get_input_embeddings(self):
        return self.model.embed_tokens

    def set_input_embeddings(self, value):
        self.model.embed_tokens = value

    def resize_token_embeddings(self, new_num_tokens: int, mean_resizing: bool = False, std: float = 0.02):
        """model.py:262.  New rows ~ N(0, std) (mean_resizing=False semantics); tied heads stay tied."""
        emb = self.model.embed_tokens
        old = emb.num_embeddings
        if new_num_tokens == old:
            return emb

        def grow(w):
            nw = torch.empty((new_num_tokens, w.shape[1]), dtype=w.dtype, device=w.device)
            n = min(old, new_num_tokens)
            nw[:n] = w.data[:n]
            if new_num_tokens > old:
                nw[old:].normal_(mean=0.0, std=std)
            return nn.Parameter(nw, requires_grad=w.requires_grad)

        self.drop_decode_weights()
        tied = self.lm_head.weight is emb.weight
        emb.weight = grow(emb.weight)
        emb.num_embeddings = new_num_tokens
        self.lm_head.weight = emb.weight if tied else grow(self.lm_head.weight)
        self.lm_head.out_features = new_num_tokens
        self.config.vocab_size = new_num_tokens
        return emb

    # -- weight-only 8-bit copies for the decode step (opt-in) -------------------------------------------
    @torch.no_grad()
    def quantize_decode_weights(self, fmt: str = "mxfp8", lm_head: bool = True):
        """Build MXFP8 copies (include/mm_hip.h: e4m3 elements, one power-of-two scale per 32 k; 1 + 1/32 byte per weight) of the
        matrices a decode step streams: per layer the fused q|k|v, o_proj, the fused gate|up (Apertus: up_proj) and down_proj, and
        (lm_head=True) the matrix lm_head reads at decode, a tied embedding included.  forward(..., decode_weights="mxfp8") then
        reads them on decode steps and forward(..., prefill_weights="mxfp8") on every other call made without autograd (the prefill);
        without those arguments, and in training always, the bf16 weights are read.  The bf16 weights stay: the copies cost
        about half their size again in HBM (~8.3 GB on the 8B model).

        The copies are plain tensors held beside the modules: absent from state_dict, checkpoints and FlatParams.  They are a
        SNAPSHOT of the weights at the time of the call.  train(True), load_state_dict / from_pretrained,
        resize_token_embeddings and .to() drop it; nothing else does -- the HIP optimiser writes parameters through raw pointers and
        does not bump `_version`, so a change of the weights cannot be detected: after any other update, call this again (or
        drop_decode_weights())."""
        if fmt != "mxfp8":
            raise ValueError(f"decode weight format {fmt!r}: only 'mxfp8' is supported")
        if self.dtype != torch.bfloat16:
            raise ValueError(f"MXFP8 decode weights need a bf16 model, this one is {self.dtype}")

        def pack(w16):
            w = w16.get().data
            if w.shape[1] % 32:
                raise ValueError(f"MXFP8 decode weights need in_features % 32 == 0, got a [{w.shape[0]}, {w.shape[1]}] matrix")
            return W8(K.quant_mxfp8(w), w.shape[0])

        self._decode_w8 = {"fmt": fmt, "layers": [{name: pack(w) for name, w in lw.items()} for lw in self._w16["layers"]],
                           "lm_head": pack(self._w16["lm_head"]) if lm_head else None}
        return self

    def drop_decode_weights(self):
        """Free the copies of quantize_decode_weights()."""
        self._decode_w8 = None

    def _linear_widths(self):
        """The input widths of the decoder layers' linears, ascending."""
        widths = {self.config.hidden_size}
        for layer in self.model.layers:
            widths |= {layer.self_attn.Hq * layer.self_attn.D, layer.mlp.I}
        return sorted(widths)

    def decode_weights_ok(self, B: int):
        """None when a decode step of B sequences can stream the MXFP8 copies, else the reason it cannot (the opt-in never falls
        back silently: generate raises it before the prefill)."""
        if self.dtype != torch.bfloat16:
            return f"model dtype is {self.dtype}, not bfloat16"
        if B > 16:
            return f"batch of {B} sequences (the weight-streaming decode step takes at most 16)"
        for Kd in self._linear_widths():
            if Kd % 32:
                return f"a weight matrix with {Kd} input features (not a multiple of 32)"
            if not K.decode_fits(B, Kd):
                return f"{B} activation rows of {Kd} features do not fit the decode kernel's LDS stage"
        return None

    def prefill_weights_ok(self, B: int, S: int, check_grad: bool = True):
        """None when a forward of B x S positions can run its decoder-layer linears as MXFP8 x MXFP8 GEMMs (forward(...,
        prefill_weights="mxfp8")), else the reason it cannot (the opt-in never falls back silently: forward and generate raise it
        before any work).  check_grad=False: the caller switches autograd off itself (generate)."""
        if self.dtype != torch.bfloat16:
            return f"model dtype is {self.dtype}, not bfloat16"
        if check_grad and torch.is_grad_enabled():
            return "autograd is enabled (the MXFP8 prefill has no backward: run it under torch.no_grad())"
        for Kd in self._linear_widths():
            why = K.gemm_mx8_supported(max(1, B * S), self.config.hidden_size, Kd)
            if why is not None:
                return f"a weight matrix with {Kd} input features: {why}"
        return None

    def train(self, mode: bool = True):
        if mode:
            self.drop_decode_weights()
        return super().train(mode)

    def _load_from_state_dict(self, *args, **kwargs):
        self.drop_decode_weights()
        return super()._load_from_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):         # .to(device / dtype): the copies would describe other tensors
        self.drop_decode_weights()
        return super()._apply(fn, *args, **kwargs)

    # -- compute --------------------------------------------------------------------------------------
    def _tables(self, position_ids):
        if self._inv_freq is None or self._inv_freq.device != position_ids.device:
            self._inv_freq = rope_inv_freq(self.config).to(position_ids.device)
        return K.rope_table(position_ids.reshape(-1).contiguous(), self._inv_freq, self.dtype == torch.bfloat16)

    def _heads_ok(self, written, kernel):
        """kv_cache_ok and samples_ok: both decode attention kernels take bf16, head_dim 128 and 1, 2 or 4 query heads per key/value
        head; `written`, `kernel`: how each reason names them."""
        c = self.config
        if self.dtype != torch.bfloat16:
            return f"model dtype is {self.dtype}, not bfloat16"
        if c.head_dim != 128:
            return f"head_dim is {c.head_dim} ({written} for 128)"
        Hq, Hkv = c.num_attention_heads, c.num_key_value_heads
        if Hq % Hkv or Hq // Hkv not in (1, 2, 4):
            return f"{Hq} query heads on {Hkv} key/value heads ({kernel} takes 1, 2 or 4 per key/value head)"
        return None

    def kv_cache_ok(self, B: int):
        """None when a batch of B sequences can keep its KV cache in MXFP8, else the reason it cannot (the opt-in never falls back
        silently: new_cache and generate raise it before the prefill)."""
        return self._heads_ok("the MXFP8 cache and its decode kernel are written", "the MXFP8 decode kernel")

    def samples_ok(self, B: int, n: int):
        """None when B prompts can be decoded as n samples each over one shared copy of the prompt's keys and values
        (LayerKVCacheShared), else the reason they cannot (the opt-in never falls back silently: new_cache and generate raise it
        before the prefill)."""
        return self._heads_ok("the shared-prefix decode kernel is written", "the shared-prefix decode kernel")

    def beams_ok(self, B: int, n: int):
        """None when B prompts can be decoded as n beams each over one shared copy of the prompt's keys and values (LayerKVCacheBeam
        and mm_beam_step), else the reason they cannot."""
        if self.config.vocab_size < 2 * n:
            return f"vocab_size is {self.config.vocab_size}: beam search draws 2 n = {2 * n} candidates per step"
        return self.samples_ok(B, n)

    def lookup_ok(self, B: int, k: int):
        """None when B sequences can be decoded with prompt-lookup drafts of k tokens -- verify steps of B (k + 1) rows through the
        weight-streaming linears and mm_attn_decode_verify over a LayerKVCacheLookup --, else the reason they cannot.  The bf16
        weights stream at any input width (mm_gemm's M <= 16 kernels; the LDS-staged, fused forms are taken where K.decode_fits says
        the rows fit: DecoderLayer.can_verify_fused).  The MXFP8 copies have the staged kernel only: with decode_weights="mxfp8" the
        width rule is decode_weights_ok(B (k + 1))'s, which generate asks as well."""
        why = self._heads_ok("the verify decode kernel is written", "the verify decode kernel")
        if why is not None:
            return why
        M = B * (k + 1)
        if M > 16:
            return f"{B} sequences x (k + 1 = {k + 1}) positions = {M} rows (a verify step is one weight-streaming launch of at most 16)"
        return None

    # option -> (the values it takes besides None; None: an int its caller has validated, the method that says why it cannot be used)
    OPTIONS = {"decode_weights": (("mxfp8",), "decode_weights_ok"), "kv_cache": (("mxfp8",), "kv_cache_ok"),
               "prefill_weights": (("mxfp8",), "prefill_weights_ok"), "samples": (None, "samples_ok"),
               "num_return_sequences": (None, "samples_ok"), "num_beams": (None, "beams_ok"), "beams": (None, "beams_ok"),
               "prompt_lookup_num_tokens": (None, "lookup_ok"), "lookup": (None, "lookup_ok")}

    def check_option(self, name, value, *args, **kw):
        """ValueError when an opt-in is given a value it does not take, or -- with the arguments of its *_ok method -- when that
        method has a reason why it cannot be used.  None (the option is off) passes."""
        allowed, ok = self.OPTIONS[name]
        if value is None:
            return
        if allowed is not None and value not in allowed:
            raise ValueError(f"{name}={value!r}: None or 'mxfp8'")
        why = getattr(self, ok)(*args, **kw) if args or kw else None
        if why is not None:
            raise ValueError(f"{name}={value!r} cannot be used: {why}")

    def new_cache(self, B, Smax, kv_cache: Optional[str] = None, samples: int = 1, prompt_len: Optional[int] = None, beams: int = 1,
                  lookup: Optional[int] = None, guided: bool = False):
        """kv_cache="mxfp8": LayerKVCacheMX8 (about half the bytes per cached position); ValueError when kv_cache_ok says it cannot.
        samples=n > 1: LayerKVCacheShared for B prompts of at most prompt_len positions and n sample rows each with room for
        Smax - prompt_len generated tokens; ValueError when samples_ok says it cannot, or together with kv_cache.
        beams=n > 1: LayerKVCacheBeam of the same sizes, every layer holding the SAME `tables` object (set tables.current to the
        step's ancestor table); ValueError when beams_ok says it cannot, or together with kv_cache or samples.
        lookup=k >= 1: LayerKVCacheLookup (prompt-lookup decoding with drafts of k tokens; Smax includes the k slots a last verify step
        may write behind the last emitted id), every layer holding the SAME `shared` object (its base / bound are the decode loop's to
        set); ValueError when lookup_ok says it cannot, or together with kv_cache, samples or beams.
        guided=True: LayerKVCacheGuided (classifier-free guidance) for B (conditional, unconditional) pairs -- 2 B rows -- of at most
        prompt_len positions each with room for Smax - prompt_len generated tokens; ValueError together with any of the others."""
        c = self.config
        if guided:
            if kv_cache is not None or samples != 1 or beams != 1 or lookup is not None:
                raise ValueError(f"guided=True with kv_cache={kv_cache!r}, samples={samples!r}, beams={beams!r}, lookup={lookup!r}: the "
                                 "guided cache is a plain one whose rows are the two halves of every pair")
            if prompt_len is None or not 1 <= int(prompt_len) <= Smax:
                raise ValueError(f"guided=True needs prompt_len in [1, Smax = {Smax}], got {prompt_len!r}")
            return [LayerKVCacheGuided(B, int(prompt_len), Smax - int(prompt_len), c.num_key_value_heads, c.head_dim, self.dtype,
                                       self.device) for _ in range(c.num_hidden_layers)]
        val = dict(lookup=lookup, beams=beams, samples=samples, kv_cache=kv_cache)
        on = dict(lookup=lookup is not None, beams=beams != 1, samples=samples != 1, kv_cache=kv_cache is not None)
        shape = (c.num_key_value_heads, c.head_dim, self.dtype, self.device)
        if not on["lookup"]:
            self.check_option("kv_cache", kv_cache, B)
        mode = None
        for name, hi, excludes, text in _CACHE_MODES:
            if name == "lookup" and lookup is None:          # the one mode that is off as None: no integer to check
                continue
            n = _int_arg(name, val[name], 1, hi)
            if on[name]:
                if any(on[other] for other in excludes):
                    raise ValueError(text.format(**val))
                self.check_option(name, n, B, n)
                mode = name
                break
        layers = range(c.num_hidden_layers)
        if mode is None:
            cls = LayerKVCache if kv_cache is None else LayerKVCacheMX8
            return [cls(B, Smax, *shape) for _ in layers]
        if mode == "lookup":
            shared = LayerKVCacheLookup.Shared()
            return [LayerKVCacheLookup(B, Smax, *shape, shared) for _ in layers]
        if prompt_len is None or not 1 <= int(prompt_len) <= Smax:
            raise ValueError(f"{mode}={n} needs prompt_len in [1, Smax = {Smax}], got {prompt_len!r}")
        Sp = int(prompt_len)
        if mode == "samples":
            return [LayerKVCacheShared(B, n, Sp, Smax - Sp, *shape) for _ in layers]
        tables = LayerKVCacheBeam.Tables()
        return [LayerKVCacheBeam(B, n, Sp, Smax - Sp, *shape, tables) for _ in layers]

    def forward(self, input_ids=None, inputs_embeds=None, attention_mask=None, position_ids=None,
                past_key_values=None, labels=None, use_cache=None, return_dict=True, logits_to_keep: int = 0,
                decode_weights: Optional[str] = None, kv_cache: Optional[str] = None, prefill_weights: Optional[str] = None, **kwargs):
        """kv_cache="mxfp8": the format of the cache this call allocates (use_cache without past_key_values); a cache handed in keeps
        its own.  decode_weights="mxfp8": a decode step (one new token per sequence over a cache, can_decode_step) streams the copies of
        quantize_decode_weights() instead of the bf16 weights; anything else (prefill, training) reads the bf16 weights -- unless
        prefill_weights="mxfp8": a call that is NOT a decode step (S > 1, or can_decode_step false) then runs every decoder-layer
        linear -- fused q|k|v (+ bias), o_proj (+ residual), fused gate|up (Apertus: up_proj), down_proj (+ residual) -- as an
        MXFP8 x MXFP8 GEMM on the block-scaled MFMA (DecoderLayer.infer, W8.linear): the same copies (built here if absent, under the
        same snapshot rule) and the linear's bf16 input quantised on the way in.  Norms, RoPE, attention, the activation, the cache
        append and the final norm stay the bf16 kernels, and lm_head -- which sees logits_to_keep rows -- keeps its bf16 weights on
        this path.  It needs autograd off (there is no backward through it) and raises ValueError with prefill_weights_ok's reason
        otherwise; on a decode step the argument is ignored (decode_weights governs those)."""
        if (input_ids is None) == (inputs_embeds is None):
            raise ValueError("You must specify exactly one of input_ids or inputs_embeds")
        self.check_option("prefill_weights", prefill_weights)
        self.check_option("decode_weights", decode_weights)
        if decode_weights is not None and (self._decode_w8 is None or self._decode_w8["fmt"] != decode_weights):
            raise ValueError("decode_weights given without copies to read: call quantize_decode_weights() first")
        if inputs_embeds is None:
            inputs_embeds = self.model.embed_tokens(input_ids)
        B, S, H = inputs_embeds.shape
        dev = inputs_embeds.device
        cache = past_key_values
        past = cache[0].positions() if cache else 0
        rows = kwargs.get("loss_rows")
        if rows is not None and (labels is None or cache or use_cache or logits_to_keep or rows.n == 0 or rows.total != B * S):
            rows = None                                      # anything but a plain training forward: every position's logits
        if use_cache and cache is None:
            cache = self.new_cache(B, S + int(kwargs.get("max_new_tokens", 512)), kv_cache=kv_cache)
        if position_ids is None:
            position_ids = (torch.arange(S, device=dev) + past).unsqueeze(0).expand(B, S)
        cos, sin = self._tables(position_ids.to(dev))
        key_mask = None
        if attention_mask is not None and past == 0 and (
                getattr(attention_mask, "_mm_all_ones", False) or (not attention_mask.is_cuda and bool(attention_mask.all()))):
            attention_mask = None       # an all-ones mask masks nothing (HF: _ignore_causal_mask_sdpa).  Known without a device
                                        # sync only for a host tensor, or from the flag DevicePrefetcher computed on the host copy
        if attention_mask is not None:
            key_mask = attention_mask.to(device=dev, dtype=torch.int64).contiguous()
        x = inputs_embeds.reshape(B * S, H)
        if not x.is_contiguous():
            x = x.contiguous()
        layers = self.model.layers
        # the plan of the call, decided once.  A step (every layer takes infer): one new token per sequence over a cache, or S = k + 1
        # positions per sequence over a prefilled LayerKVCacheLookup (a prompt-lookup verify step); fused where every layer can fold
        # its norms and SwiGLU into the weight-streaming launches.  The MXFP8 prefill (every layer takes infer).  None: training and
        # everything else (every layer takes forward)
        plan = None
        verify = bool(cache and len(layers) and isinstance(cache[0], LayerKVCacheLookup) and past)
        if verify:
            if x.dtype != torch.bfloat16 or torch.is_grad_enabled() or B * S > 16:
                raise ValueError(f"a verify step of {B} x {S} {x.dtype} rows on a prompt-lookup cache: bf16, at most 16 rows, no autograd")
            plan = Plan("step", all(layer.can_verify_fused(x, B * S) for layer in layers))
        elif cache and len(layers):
            if all(layer.can_decode_step_fused(x, B, S, c) for layer, c in zip(layers, cache)):
                plan = Plan("step", True)
            elif all(layer.can_decode_step(x, B, S, c) for layer, c in zip(layers, cache)):
                plan = Plan("step", False)
        w = self._decode_w8 if plan and decode_weights is not None else self._w16      # steps alone read decode_weights
        if prefill_weights is not None and not plan and len(layers):
            self.check_option("prefill_weights", prefill_weights, B, S)
            if self._decode_w8 is None or self._decode_w8["fmt"] != prefill_weights:
                self.quantize_decode_weights(prefill_weights)
            plan, w, rows = Plan("prefill", False), self._decode_w8, None
        if plan:
            for i, layer in enumerate(layers):
                x = layer.infer(w["layers"][i], x, cos, sin, key_mask, B, S, cache[i] if cache else None, plan)
        else:
            # training step (Trainer.compute_loss hands over `loss_rows`): the loss and every gradient depend only on the rows whose
            # shifted label is not -100 (HF:loss/loss_utils.py:36-71 ignores the others; their dlogits are exactly zero), so the
            # final norm, lm_head and the loss -- and what follows attention in the LAST layer -- run on those rows alone;
            # `logits` is then not returned
            last = len(layers) - 1
            for i, layer in enumerate(layers):
                x = layer(x, cos, sin, key_mask, B, S, cache=cache[i] if cache else None, rows=rows if i == last else None)
            if rows is not None and not len(layers):
                x = Fm.rows_select(x, rows)
        # on a fused step every RMSNorm is applied by the projection that consumes it, the final norm by lm_head -- when lm_head
        # sees the rows the layers returned (a decode step's one position per sequence, or every position of a verify step)
        fused_head = (bool(plan) and plan.fused and not (verify and logits_to_keep)
                      and self.lm_head.bias is None and self.model.norm.bias is None)
        if not fused_head:
            x, _ = self.model.norm(x)
        V = self.config.vocab_size
        if logits_to_keep:
            x = x.view(B, S, H)[:, -logits_to_keep:, :].reshape(-1, H)
            Sk = logits_to_keep
        else:
            Sk = S
        # a step reads lm_head's copy when decode_weights made one; everything else the module (autograd, bf16 weights)
        head = (w["lm_head"] or self._w16["lm_head"]) if plan and plan.rows == "step" else None
        if fused_head:
            logits2d = head.stream(x, None, self.model.norm.weight, self.model.norm.eps, True)
        elif head is not None:                                   # a decode step: lm_head's copy, when decode_weights made one
            logits2d = head.linear(x, ldc_pad=True)
        else:
            logits2d = self.lm_head(x, ldc_pad=True)             # [B*Sk, V] view, row stride padded to 64
        loss = None
        if rows is not None:
            loss = Fm.causal_lm_loss(logits2d, V, rows.labels)
            out = CausalLMOutput(loss=loss, logits=None, past_key_values=None)
            return out if return_dict else (loss, None, None)
        if labels is not None:
            shift = torch.nn.functional.pad(labels.to(dev), (0, 1), value=-100)[..., 1:].reshape(-1).contiguous()
            loss = Fm.causal_lm_loss(logits2d, V, shift)
        logits = logits2d.as_strided((B, Sk, V), (Sk * logits2d.stride(0), logits2d.stride(0), 1))
        out = CausalLMOutput(loss=loss, logits=logits, past_key_values=cache if use_cache else None)
        return out if return_dict else (loss, logits, out.past_key_values)

    __call__ = nn.Module.__call__
