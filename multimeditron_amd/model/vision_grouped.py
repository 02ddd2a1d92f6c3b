"""E vision towers of equal shape as ONE chain of grouped launches (the MoE image modalities' experts, opt-in through
`grouped_towers`): the expert is a batch dimension of every kernel instead of E chains of ~1,200 launches each.

Activations are expert-major [E * n * T, C].  The ops whose operands differ per expert (the Linears and LayerNorms) take the
experts' parameters as lists and run one grouped launch (functional.GroupedLinearFn / GroupedLayerNormFn); everything else in
`VisionLayer.forward` carries no per-expert operand and runs once with batch E * n: attention, head padding, the GELU backward,
`drop_cls`.  The embedding stage runs once per tower, not once per layer, and stays E calls.  Same kernels' arithmetic as the
per-expert towers, so the results are theirs bit for bit (the fp32 attention backward's atomics aside).

Ordinary autograd: no graph capture, no side streams, no state between calls."""
from __future__ import annotations

from typing import List, Optional

import torch

from .. import functional as Fm
from .._lib import GROUP_MAX
from ..nn import fire_forward_pre_hooks, grad_dummy
from .vision import attention_core


def ineligible(experts) -> Optional[str]:
    """None when the experts can run as one grouped chain, else the reason they cannot."""
    experts = list(experts)
    if len(experts) > GROUP_MAX:
        return f"{len(experts)} experts (a grouped launch takes at most {GROUP_MAX})"
    cfg0 = experts[0].config
    p0 = experts[0].embeddings.position_embedding.weight
    for ex in experts:
        if ex.config != cfg0:
            return "the experts' vision configs differ"
        for p in ex.parameters():
            if p.dtype != p0.dtype:
                return "the experts' dtypes differ"
            if not p.is_cuda or p.device != p0.device:
                return "the experts are not all on one GPU"
    return None


def _norm(norms, x):
    return Fm.grouped_layernorm(x, [m.weight for m in norms], [m.bias for m in norms], norms[0].eps, dummy=grad_dummy(norms[0].weight))


def _linear(lins, x, residual=None, act=0):
    return Fm.grouped_linear(x, [m.weight for m in lins], [m.bias for m in lins], residual=residual, act=act,
                             dummy=grad_dummy(lins[0].weight))


def _layer(layers, x, B, T):
    """VisionLayer.forward for E experts at once; B = E * n images."""
    for l in layers:
        fire_forward_pre_hooks(l)
    a0 = layers[0].self_attn
    h, x = _norm([l.layer_norm1 for l in layers], x)
    qkv = Fm.grouped_linear(h, [l.self_attn._wqkv for l in layers], [l.self_attn._bqkv for l in layers],
                            dummy=grad_dummy(a0.q_proj.weight))
    x = _linear([l.self_attn.out_proj for l in layers], attention_core(qkv, B, T, a0.heads, a0.hd), residual=x)
    h, x = _norm([l.layer_norm2 for l in layers], x)
    h = _linear([l.mlp.fc1 for l in layers], h, act=layers[0].mlp.act)
    return _linear([l.mlp.fc2 for l in layers], h, residual=x)


def grouped_towers(experts, pixels) -> List[torch.Tensor]:
    """Every expert tower on the same pixels -> E token tensors [n, P, C] (CLS dropped for CLIP towers), as E calls of
    `expert(pixels).last_hidden_state` followed by `drop_cls` give them."""
    experts = list(experts)
    E, n = len(experts), pixels.shape[0]
    cfg = experts[0].config
    T = cfg.num_tokens
    for ex in experts:
        fire_forward_pre_hooks(ex, recurse=False)
    xs = [ex.embeddings(pixels) for ex in experts]             # once per tower; __call__: the embeddings' own hooks fire
    x = torch.cat(xs, dim=0)                                   # expert-major [E * n * T, C]
    if experts[0].pre_layrnorm is not None:
        norms = [ex.pre_layrnorm for ex in experts]
        for m in norms:
            fire_forward_pre_hooks(m)
        x, _ = _norm(norms, x)
    for i in range(cfg.num_hidden_layers):
        x = _layer([ex.encoder.layers[i] for ex in experts], x, E * n, T)
    if experts[0].post_layernorm is not None:
        norms = [ex.post_layernorm for ex in experts]
        for m in norms:
            fire_forward_pre_hooks(m)
        x, _ = _norm(norms, x)
    C = x.shape[-1]
    x = Fm.drop_cls(x, E * n, T)                               # [E * n, T - 1, C], as expert_towers.run_experts' per-expert tower does
    P = x.shape[1]
    return list(x.view(E, n, P, C).unbind(0))
