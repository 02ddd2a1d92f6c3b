"""`moe_meditron_clip` and `moe_meditron_clip_pep`: the mixture-of-experts image modalities (reference
model/modalities/image_modality_moe.py:10-246, image_modality_moe_pep.py:11-288 and model/attention.py:5-101) on libmmhip kernels.

E CLIP vision towers ("experts") run on every image; a gating network scores the image; one of three fusions combines the
experts' patch tokens; the MLP projector maps them into the LLM's embedding space:

    sequence_append   [n, E*P, C]  all experts' tokens one after the other                          (:165-168)
    weighted_average  [n, P, C]    sum_e w[n,e] * tokens_e                                           (:169-176)
    cross_attn        [n, P, C]    generalist tokens attend over the specialists' tokens, each scaled by the softmax of the
                                   specialists' gate weights (CrossAttention, attention.py:48-101)  (:177-203)

What runs where: the towers are this package's `VisionTransformer` (model/vision.py), the fusion is `mm_expert_fuse`, the
cross-attention is three biased GEMMs + the non-causal flash-attention kernel (Nq = P queries over (E-1)*P keys) + a GEMM.
Parameter names equal the reference's (`experts.{e}.*`, `cross_attn.{q,k,v}_proj / proj`, `projector.projection.{0,2,4}`).

`moe_meditron_clip_pep` (per-expert projection) gives every expert its own MLP projector (`projectors.{e}.projection.{0,2,4}`)
and fuses in the LLM's embedding space; its cross-attention therefore has `hidden_size / cross_attn_heads`-wide heads: 512 in the
shipped recipe (cookbook/sft/moe/*/attn/pep: 4096 / 8), 96 in the shared-projector one (768 / 8).  Neither is a flash-kernel
width; both run on the one-pass cross-attention kernel `mm_xattn_*` (csrc/mm_xattn.hip: up to 1024 keys, head widths up to 512).

The gate (reference moe/gating.py:37-89, a torchvision ResNet-50 with an E-way fc) is `modalities/gating.py`: the same key set
on libmmhip's NHWC convolution kernels, built from `config.gating_path` when that is a directory holding a `config.json`
(`GatingNetwork.from_pretrained`), as the submodule `gating_network`: by default frozen, eval mode always, outside the optimiser.  A
`gating_network=` argument wins over the path, and may be any callable with the reference's output contract
`pixels [n,3,H,W] -> (logits [n,E], topk_indices, weights [n,E])`.  Training the gate in FULL mode (train-mode BatchNorm, a ResNet
backward, a gradient through the fusion weights) is opt-in through the config field `train_gate`.  The experts run side by side, each on its own HIP
stream or replayed from captured hipGraphs (model/expert_towers.py: `run_experts` picks the path), or -- opt-in through the config field `grouped_towers` / MM_MOE_GROUPED=1 -- as ONE chain of grouped
launches with the expert as a batch dimension (model/vision_grouped.py: no graph capture, no side streams).  `CrossAttention`'s two dropouts
(p = 0.1 on the attention probabilities and on the output projection, active in the reference whenever the module trains) are
Philox-based: eval mode equals the reference, train mode equals it in distribution (torch's generator cannot be reproduced)."""
from __future__ import annotations

from typing import Any, Callable, Dict, List, Optional

import torch
import torch.nn as nn

from ... import functional as Fm
from ...nn import Linear, grad_dummy
from ..constants import MODALITY_VALUE_KEY, NUM_EMBEDDINGS_KEY
from ..expert_towers import run_experts
from ..presets import resolve_preprocessor_config, resolve_vision_config
from ..projectors.mlp import MLPProjector
from ..vision import VisionConfig, VisionTransformer
from .base import AutoModality, BaseModality, BaseModalityConfig, BaseModalityProcessor
from .gating import GatingNetwork, is_gate_dir
from .image_modality import ClipImagePreprocessor


class MOEImageConfig(BaseModalityConfig):
    """reference image_modality_moe.py:10-52 (same arguments)."""

    def __init__(self, hidden_size: int = 1024, use_bias_proj: bool = True, expert_clip_names: Optional[List[str]] = None,
                 image_processor: str = "openai/clip-vit-large-patch14", gating_path: str = "", top_k_experts: int = 1,
                 projection_type: str = "mlp", generalist_idx: int = -1, fusion_method: str = "weighted_average",
                 cross_attn_heads: int = 8, train_gate: bool = False, grouped_towers: bool = False, **kwargs):
        super().__init__(modality_type="image", hidden_size=hidden_size)
        self.grouped_towers = bool(grouped_towers)       # opt-in: the expert towers as one chain of grouped launches (vision_grouped.py)
        self.train_gate = bool(train_gate)       # opt-in: unfreezing the modality also trains the gating network (the reference's FULL mode)
        self.use_bias_proj = use_bias_proj
        self.expert_clip_names = list(expert_clip_names or [])
        self.top_k_experts = top_k_experts
        self.gating_path = gating_path
        self.projection_type = projection_type
        self.image_processor = image_processor
        self.generalist_idx = generalist_idx
        self.fusion_method = fusion_method
        self.cross_attn_heads = cross_attn_heads

    def to_dict(self) -> Dict[str, Any]:
        d = super().to_dict()
        for key in ("train_gate", "grouped_towers"):     # written only when set: configs saved without them stay byte-identical
            if not d.get(key):
                d.pop(key, None)
        return d


class MOEImageProcessor(BaseModalityProcessor):
    """reference image_modality_moe.py:55-88: CLIP preprocessing; the number of placeholder tokens depends on the fusion."""

    def __init__(self, config: MOEImageConfig):
        super().__init__(config)
        vis = VisionConfig.from_dict(resolve_vision_config(config.image_processor))
        self.image_processor = ClipImagePreprocessor(resolve_preprocessor_config(config.image_processor, vis.image_size))
        self._num_patches_per_entry = vis.num_patches
        self.top_k_experts = config.top_k_experts
        self.fusion_method = config.fusion_method

    def process(self, modality: Dict[str, Any]) -> Dict[str, Any]:
        out = modality.copy()
        out[MODALITY_VALUE_KEY] = self.image_processor(modality[MODALITY_VALUE_KEY])
        if self.fusion_method == "sequence_append":
            out[NUM_EMBEDDINGS_KEY] = self._num_patches_per_entry * self.top_k_experts
        elif self.fusion_method in ("weighted_average", "cross_attn"):
            out[NUM_EMBEDDINGS_KEY] = self._num_patches_per_entry
        else:
            raise ValueError(f"Unknown fusion_method: {self.fusion_method}")
        return out


class CrossAttention(nn.Module):
    """reference model/attention.py:5-101.  `attn_drop` acts on the attention probabilities and `proj_drop` on the output of
    `proj`, both only while the module trains (nn.Dropout semantics); the masks come from Philox streams keyed by torch's seed
    (functional.next_dropout_stream), so they differ from torch's own generator draw for draw: eval mode equals the reference,
    train mode equals it in distribution (tests/test_xattn_gpu.py holds the kernels to a torch restatement on the SAME mask)."""

    def __init__(self, dim: int, num_heads: int = 8, qkv_bias: bool = False, attn_drop: float = 0.1, proj_drop: float = 0.1,
                 dtype=None, device=None):
        super().__init__()
        assert dim > 0 and dim % num_heads == 0, "dim must be divisible by num_heads"
        self.num_heads, self.head_dim = num_heads, dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.q_proj = Linear(dim, dim, bias=qkv_bias, dtype=dtype, device=device)
        self.k_proj = Linear(dim, dim, bias=qkv_bias, dtype=dtype, device=device)
        self.v_proj = Linear(dim, dim, bias=qkv_bias, dtype=dtype, device=device)
        self.proj = Linear(dim, dim, dtype=dtype, device=device)
        self.attn_drop_p, self.proj_drop_p = attn_drop, proj_drop
        self._wkv = Fm.ParamGroup([self.k_proj.weight, self.v_proj.weight])       # one GEMM for K and V
        self._bkv = Fm.ParamGroup([self.k_proj.bias, self.v_proj.bias]) if qkv_bias else None

    def forward(self, x: torch.Tensor, context: torch.Tensor) -> torch.Tensor:
        """x [n, Nq, C] queries, context [n, Nkv, C] (the specialists' tokens, already concatenated along the sequence)."""
        from ... import kernels as K
        n, Nq, C = x.shape
        Nkv = context.shape[1]
        h, d = self.num_heads, self.head_dim
        drop = self.attn_drop_p if self.training else 0.0
        q = self.q_proj(x.reshape(n * Nq, C))
        kv = Fm.linear(context.reshape(n * Nkv, C), self._wkv, self._bkv, dummy=grad_dummy(self.k_proj.weight))
        if K.xattn_supported(x.dtype, Nkv, d):
            # the one-pass kernel: any head width up to 512 (the shipped recipes: 768 / 8 = 96 and 4096 / 8 = 512), up to 1024 keys, dropout inside
            o = Fm.cross_attention(q, kv, n, Nq, Nkv, h, d, self.scale, drop)
        else:
            # more than 1024 keys: the flash kernels, narrower heads zero-padded to 64 / 128 as the SigLIP tower's are
            if drop > 0.0 and not getattr(CrossAttention, "_warned_no_attn_drop", False):
                import warnings
                CrossAttention._warned_no_attn_drop = True      # far outside the reference's recipes (P = 49, E = 5: 196 keys; four ViT-L/14
                                                                # experts: 1024, which mm_xattn_* takes with its dropout); say so, once
                warnings.warn(f"CrossAttention over {Nkv} keys runs on the flash kernels, which have no attention-probability dropout "
                              f"(mm_xattn_* holds <= 1024 keys per query): attn_drop = {drop} is NOT applied; proj_drop still is.")
            hw = Fm.attention_head_width(d, x.dtype)
            if hw != d:
                q, kv = Fm.head_pad(q, h, d, hw), Fm.head_pad(kv, 2 * h, d, hw)
            o = Fm.cross_attention(q, kv, n, Nq, Nkv, h, hw, self.scale, 0.0)
            if hw != d:
                o = Fm.head_strip(o, h, d, hw)
        o = self.proj(o)
        return Fm.dropout(o, self.proj_drop_p, self.training).view(n, Nq, C)


def _resolve_gate(config, gating_network, dtype, device):
    """The `gating_network=` argument wins; otherwise a `gating_path` that is a directory with a config.json is the reference's
    `GatingNetwork.from_pretrained(config.gating_path)` (image_modality_moe.py:123), in the modality's dtype and device; anything
    else leaves the plug empty."""
    if gating_network is None and is_gate_dir(getattr(config, "gating_path", None)):
        gating_network = GatingNetwork.from_pretrained(config.gating_path, dtype=dtype, device=device)
    return gating_network


_NO_GATE = ("{cls} needs a gating network: set `gating_path` to a directory written by GatingNetwork.save_pretrained / the "
            "reference (config.json + model.safetensors, keys resnet.*), or assign `modality.gating_network = fn` with "
            "fn(pixels [n,3,H,W]) -> (logits, topk_indices, weights [n, E]) (reference moe/gating.py:73-89).")


class _FrozenGate:
    """By default the gate stays frozen and in eval mode whatever the training mode.  The reference trains it in FULL mode
    (image_modality_moe.py:233-241); here that is opt-in: with `config.train_gate`, unfreezing the modality's embedder makes a
    `GatingNetwork` trainable (train-mode BatchNorm, gradients through the fusion weights) and freezing it reverses that
    (DESIGN.md section 7).  A callable plug is left alone."""
    _warned_frozen_gate = False

    def _gate_trains(self):
        return bool(getattr(self.config, "train_gate", False)) and isinstance(getattr(self, "gating_network", None), GatingNetwork)

    def _set_gate_trainable(self, flag: bool):
        self.gating_network.set_trainable(flag)
        self.gating_network.train(flag)

    def _keep_gate_frozen(self, warn=False):
        """the default: eval mode, no gradient; a `train_gate` modality's gate is left as its last freeze / unfreeze set it"""
        g = getattr(self, "gating_network", None)
        if not isinstance(g, nn.Module) or self._gate_trains():
            return
        g.eval()
        for p in g.parameters():
            p.requires_grad = False
        if warn and not _FrozenGate._warned_frozen_gate:
            import warnings
            _FrozenGate._warned_frozen_gate = True
            warnings.warn("the MoE gating network stays frozen (eval-mode BatchNorm, no gradient): training the gate is not built")

    def _on_unfreeze(self):
        """the embedder was unfrozen: with `train_gate` the gate joins it, otherwise it stays frozen (and says so once)"""
        if self._gate_trains():
            self._set_gate_trainable(True)
        else:
            self._keep_gate_frozen(warn=True)

    def _on_freeze(self):
        if self._gate_trains():
            self._set_gate_trainable(False)
        else:
            self._keep_gate_frozen()

    def train(self, mode: bool = True):
        super().train(mode)
        self._keep_gate_frozen()
        return self

    def unfreeze_all(self):
        super().unfreeze_all()
        if self._gate_trains():
            self._on_unfreeze()
        else:
            self._keep_gate_frozen()


class _MOEImageBase(_FrozenGate, BaseModality):
    """What the two MoE image modalities share: the experts, the gate and its class-order -> expert-order permutation, freezing,
    and the three-way fusion.  A subclass states which VisionConfig fields the experts must share (`_same`, `_mismatch`), where its
    projector(s) sit (`_add_expert` / `_build_projection`, `_post`, `_project`), which order of the gate's weights
    `weighted_average` takes (`_fusion_weights`), and the texts of its errors (`_mismatch`, `_no_experts`)."""
    _post = None                    # post(e, tokens): applied to every expert's tokens before the fusion

    def __init__(self, config: MOEImageConfig, dtype: torch.dtype = torch.bfloat16, device=None, gating_network: Optional[Callable] = None):
        super().__init__(config, dtype=dtype)
        self.expert_names: List[str] = list(config.expert_clip_names)
        assert len(self.expert_names) > 0, self._no_experts
        self.experts = nn.ModuleList()
        vis0 = None
        for name in self.expert_names:
            vis = VisionConfig.from_dict(resolve_vision_config(name))
            vis0 = vis0 or vis
            if any(getattr(vis, k) != getattr(vis0, k) for k in self._same):
                raise ValueError(self._mismatch)
            self._add_expert(vis, config, dtype, device)
        self._num_patches_per_entry = vis0.num_patches
        self.generalist_idx = config.generalist_idx
        self.fusion_method = config.fusion_method.replace("-", "_")
        gating_network = _resolve_gate(config, gating_network, dtype, device)
        self.gating_network = gating_network
        names = list(getattr(getattr(gating_network, "config", None), "class_names", []) or [])
        if names:                                                        # reference :118-131: gate class order -> expert order
            lookup = {nm: i for i, nm in enumerate(self.expert_names)}
            try:
                perm = [lookup[nm] for nm in names]
            except KeyError as e:
                raise ValueError(f"Gating class name {e} not found in expert_clip_names: {self.expert_names}")
        else:
            perm = list(range(len(self.experts)))
        self.register_buffer("_gating_to_expert_perm", torch.tensor(perm, dtype=torch.long), persistent=False)
        self._build_projection(vis0, config, dtype, device)              # sets `embedding_size`, the width the LLM sees
        if self.fusion_method == "cross_attn":
            self.cross_attn = CrossAttention(self.embedding_size, num_heads=config.cross_attn_heads, qkv_bias=True, dtype=dtype, device=device)
        self.modality_frozen = not self.training

    def _add_expert(self, vis, config, dtype, device):
        self.experts.append(VisionTransformer(vis, dtype, device))       # = the reference's `expert_model.vision_model`

    @property
    def device(self):
        return self.experts[0].embeddings.patch_embedding.weight.device

    def _gate(self, pixels: torch.Tensor) -> torch.Tensor:
        """-> the gate's weights [n, E], fp32 on the device, in the gate's own class order"""
        if self.gating_network is None:
            raise NotImplementedError(_NO_GATE.format(cls=type(self).__name__))
        _logits, _topk, weights = self.gating_network(pixels)
        return weights.to(device=self.device, dtype=torch.float32)

    def _expert_order(self, w: torch.Tensor) -> torch.Tensor:
        return w.index_select(-1, self._gating_to_expert_perm.to(w.device)).contiguous()

    def gate_weights(self, pixels: torch.Tensor) -> torch.Tensor:
        return self._expert_order(self._gate(pixels))                    # reference :171-173, :185-186

    def forward(self, inputs, stages=None) -> torch.Tensor:
        pixels = torch.stack(list(inputs), dim=0) if not torch.is_tensor(inputs) else inputs
        pixels = pixels.to(self.device, non_blocking=True)
        n, E = pixels.shape[0], len(self.experts)
        w_avg, w_expert = self._fusion_weights(pixels)                    # [n, E] fp32; the gate runs before the towers
        # every expert on every image (reference :156-160)
        feats = run_experts(self.experts, pixels, post=self._post, grouped=getattr(self.config, "grouped_towers", False))
        stacked = torch.stack(feats, dim=0)                               # [E, n, P, C] (device copy; autograd unbinds it)
        P, C = stacked.shape[2], stacked.shape[3]
        if self.fusion_method == "sequence_append":
            fused = stacked.permute(1, 0, 2, 3).reshape(n, E * P, C)
        elif self.fusion_method == "weighted_average":
            fused = Fm.expert_fuse(stacked, w_avg, list(range(E)), 0)
        elif self.fusion_method == "cross_attn":
            gi = self.generalist_idx % E
            spec = [i for i in range(E) if i != gi]
            ctx = Fm.expert_fuse(stacked, w_expert(), spec, 1)            # [n, (E-1)*P, C], each specialist scaled by its weight
            fused = self.cross_attn(stacked[gi], ctx)
        else:
            raise ValueError(f"Unsupported fusion_method: {self.fusion_method}")
        fused = fused.contiguous()
        out = self._project(fused)
        if stages is not None:
            stages["moe_fused"] = fused
            stages["projector_out"] = out
        return out

    def _set_experts_trainable(self, flag: bool):
        for e in self.experts:
            for p in e.parameters():
                p.requires_grad = flag
        self.modality_frozen = not flag

    def freeze_modality_embedder(self):
        self._set_experts_trainable(False)
        self._on_freeze()

    def unfreeze_modality_embedder(self):
        self._set_experts_trainable(True)
        self._on_unfreeze()


@AutoModality.register("moe_meditron_clip")             # applied last: the config class keeps the reference's model_type
@AutoModality.register("moe_meditron_clip_shared")      # alias: the name the shipped recipes use (cookbook/sft/moe/*/*/shared/config.yaml),
class MOEImageModality(_MOEImageBase):                  # which the reference itself does not register (image_modality_moe.py:89)
    """experts -> fusion in the towers' width -> ONE projector"""
    config_class = MOEImageConfig
    preprocessor_class = MOEImageProcessor
    _same = ("hidden_size", "num_patches")
    _mismatch = "every expert must produce the same [patches, width] token grid"      # reference :166 comment
    _no_experts = "config.expert_clip_names must be non-empty"

    def _build_projection(self, vis0, config, dtype, device):
        self.embedding_size = vis0.hidden_size
        self.projector = MLPProjector(self.embedding_size, config.hidden_size, dtype=dtype, device=device)

    def _fusion_weights(self, pixels):
        w = self.gate_weights(pixels)                                     # expert order for both fusions, permuted on every forward
        return w, lambda: w

    def _project(self, fused):
        return self.projector(fused)

    def unfreeze_projection(self):
        for p in self.projector.parameters():
            p.requires_grad = True


class MOEImageConfigPEP(MOEImageConfig):
    """reference image_modality_moe_pep.py:11-52 (same arguments; its defaults)."""

    def __init__(self, hidden_size: int = 4096, use_bias_proj: bool = True, expert_clip_names: Optional[List[str]] = None,
                 image_processor: str = "openai/clip-vit-base-patch32", gating_path: str = "", top_k_experts: int = 5,
                 projection_type: str = "mlp", generalist_idx: int = -1, fusion_method: str = "weighted_average",
                 cross_attn_heads: int = 8, **kwargs):
        super().__init__(hidden_size=hidden_size, use_bias_proj=use_bias_proj, expert_clip_names=expert_clip_names,
                         image_processor=image_processor, gating_path=gating_path, top_k_experts=top_k_experts,
                         projection_type=projection_type, generalist_idx=generalist_idx, fusion_method=fusion_method,
                         cross_attn_heads=cross_attn_heads, **kwargs)


class MOEImageProcessorPEP(MOEImageProcessor):
    """reference image_modality_moe_pep.py:55-88 (identical to the shared-projector processor)."""


@AutoModality.register("moe_meditron_clip_pep")
class MOEImageModalityPEP(_MOEImageBase):
    """reference image_modality_moe_pep.py:91-288: experts -> one projector PER expert -> fusion in the projected space."""
    config_class = MOEImageConfigPEP
    preprocessor_class = MOEImageProcessorPEP
    _same = ("image_size", "patch_size")                                 # reference :131-137
    _mismatch = "sequence_append requires identical (image_size, patch_size) across experts."
    _no_experts = "No experts provided in config.expert_clip_names."

    def _add_expert(self, vis, config, dtype, device):
        super()._add_expert(vis, config, dtype, device)
        if config.projection_type != "mlp":
            raise ValueError(f"Unsupported projection_type: {config.projection_type}")
        if "projectors" not in self._modules:
            self.projectors = nn.ModuleList()
        self.projectors.append(MLPProjector(vis.hidden_size, config.hidden_size, dtype=dtype, device=device))

    def _build_projection(self, vis0, config, dtype, device):
        self.embedding_size = config.hidden_size                         # post-projection width seen by the LLM (:252-254)

    def _post(self, e, tok):
        return self.projectors[e](tok)                                    # [n, P, H]

    def _fusion_weights(self, pixels):
        w_raw = self._gate(pixels).contiguous()                           # gate order, as weighted_average uses it (:214)
        return w_raw, lambda: self._expert_order(w_raw)                   # expert order for cross_attn only, after the towers (:229-230)

    def _project(self, fused):
        return fused

    def unfreeze_projection(self):
        for p in self.projectors.parameters():
            p.requires_grad = True
