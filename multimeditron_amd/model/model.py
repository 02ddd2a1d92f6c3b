"""Drop-in for the reference's `multimeditron.model.model` (model.py:17-673): `ChatTemplate`, `MultimodalConfig`,
`MultiModalModelForCausalLM` (forward / generate / freeze policies / processors) and `bootstrap`, with the whole
numerical path -- modality encoder, projector, embed-splice, decoder, loss -- on libmmhip (gfx950) kernels.

Differences from the reference that a caller can observe (all documented in DESIGN.md):
  * the LLM and the CLIP tower are this package's own modules (model/llm.py, model/vision.py), not HF classes;
    parameter names are identical so checkpoints interchange; hub names resolve to built-in shape presets;
  * `forward` returns a small dataclass with `.loss`, `.logits`, `.past_key_values` (HF `CausalLMOutputWithPast` shape);
    `.logits` is a [B,S,V] view whose row stride is padded to a multiple of 64 elements;
  * there is no eager/CPU fallback: without libmmhip.so and a GPU every compute call raises."""
from __future__ import annotations

import json
import logging
import math
import os
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Union

import torch
import torch.nn as nn

from .. import functional as Fm
from .. import kernels as K
from ..nn import FlatParams, grad_dummy
from ..utils import get_torch_dtype, trace_range
from .decoding import BeamSearch, PromptLookup, Sampling
from .llm import XIELU, CausalLM, CausalLMOutput, LLMConfig
from .modalities import AutoModality, BaseModality, BaseModalityConfig, BaseModalityProcessor
from .presets import resolve_llm_config

logger = logging.getLogger(__name__)


@dataclass
class ChatTemplate:
    """Role delimiters + special tokens per LLM family (reference model.py:17-99)."""
    name: str = "custom"
    delimiters: Dict[str, Dict[str, str]] = field(default_factory=dict)
    special_tokens: Dict[str, str] = field(default_factory=dict)

    _IMAGE_TOKENS = {"image_start": "<|image_start|>", "image_end": "<|image_end|>"}

    @staticmethod
    def from_name(name: str) -> "ChatTemplate":
        makers = {"llama": ChatTemplate.llama, "apertus": ChatTemplate.apertus, "qwen3": ChatTemplate.qwen3}
        if name not in makers:
            raise ValueError(f"Unknown chat template name: {name}")
        return makers[name]()

    @staticmethod
    def _make(name, roles):
        return ChatTemplate(name=name, delimiters={r: {"start": s, "end": e} for r, (s, e) in roles.items()},
                            special_tokens=dict(ChatTemplate._IMAGE_TOKENS))

    @staticmethod
    def llama() -> "ChatTemplate":
        hdr = "<|start_header_id|>{}<|end_header_id|>"
        return ChatTemplate._make("llama", {r: (hdr.format(r), "<|eot_id|>") for r in ("system", "user", "assistant")})

    @staticmethod
    def apertus() -> "ChatTemplate":
        return ChatTemplate._make("apertus", {r: (f"<|{r}_start|>", f"<|{r}_end|>")
                                              for r in ("system", "developer", "user", "assistant")})

    @staticmethod
    def qwen3() -> "ChatTemplate":
        return ChatTemplate._make("qwen3", {r: (f"<|im_start|>{r}", "<|im_end|>") for r in ("system", "user", "assistant")})


class MultimodalConfig:
    """reference model.py:103-202 (same constructor arguments and dict layout)."""
    model_type = "multimodal"

    def __init__(self, vocab_size: Optional[int] = None, modalities: List[BaseModalityConfig] = (), pad_token_idx: int = 0,
                 eos_token_idx: int = 0, padding_side: str = "left", initializer_range: float = 0.02,
                 llm_path: str = "meta-llama/Llama-3.1-8B-Instruct", truncation: bool = False,
                 max_sequence_length: Optional[int] = None, dtype="bfloat16", **kwargs):
        self.vocab_size = vocab_size
        self.modalities = list(modalities)
        self.pad_token_idx = pad_token_idx
        self.eos_token_idx = eos_token_idx
        self.padding_side = padding_side
        self.initializer_range = initializer_range
        self.llm_path = llm_path
        self.dtype = dtype
        self.truncation = truncation
        self.max_sequence_length = max_sequence_length
        for k, v in kwargs.items():
            setattr(self, k, v)

    def to_dict(self):
        out = {k: v for k, v in self.__dict__.items() if not k.startswith("_") and k != "modalities"}
        out["dtype"] = str(out["dtype"]).replace("torch.", "")
        out["model_type"] = self.model_type
        out["modalities"] = [m.to_dict() for m in self.modalities]
        return out

    @classmethod
    def from_dict(cls, config_dict, **kwargs):
        d = dict(config_dict)
        d.pop("model_type", None)
        d.pop("torch_dtype", None)
        mods = [AutoModality.config_from_dict(m) for m in d.pop("modalities", [])]
        d.update(kwargs)
        return cls(modalities=mods, **d)

    def save_pretrained(self, path):
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(self.to_dict(), f, indent=2, sort_keys=True, default=str)


class MultiModalModelForCausalLM(nn.Module):
    config_class = MultimodalConfig
    base_model_prefix = "model"
    supports_gradient_checkpointing = True

    def __init__(self, config: MultimodalConfig, bootstrap=False, device=None, llm_config: Optional[dict] = None):
        """`bootstrap` is accepted for signature parity (model.py:226-230): there is no hub here, so both branches build
        the LLM from `config.llm_path`'s config.json / preset with random init; local weights are loaded by
        `load_state_dict` / `from_pretrained`."""
        super().__init__()
        self.config = config
        dtype = get_torch_dtype(config.dtype)
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self._llm_cfg = LLMConfig.from_dict(llm_config if llm_config is not None else resolve_llm_config(config.llm_path))
        self.model = CausalLM(self._llm_cfg, dtype=dtype, device=device)
        self.modalities_by_type: Dict[str, BaseModality] = {}
        self.processors_by_type: Dict[str, BaseModalityProcessor] = {}
        self.modalities_with_projection = nn.ModuleList()
        for mc in config.modalities:
            modality = AutoModality.model_from_config(mc, dtype=dtype, device=device)
            processor = AutoModality.preprocessor_from_name(mc.model_type, mc)
            if mc.modality_type in self.modalities_by_type:
                raise ValueError(f"Modality type {mc.modality_type} has already been registered")
            self.modalities_by_type[mc.modality_type] = modality
            self.processors_by_type[mc.modality_type] = processor
            self.modalities_with_projection.append(modality)
        self.apply(self._init_weights)
        if config.vocab_size is not None:
            self.model.resize_token_embeddings(config.vocab_size, mean_resizing=False, std=config.initializer_range)
        self._flat: Optional[FlatParams] = None

    # ------------------------------------------------------------------ init / packing
    def _init_weights(self, module):
        """model.py:287-308: N(0, initializer_range) weights, zero biases; norms keep (1, 0)."""
        from ..nn import Embedding, Linear, Norm
        std = self.config.initializer_range
        with torch.no_grad():
            if isinstance(module, Linear):
                module.weight.normal_(mean=0.0, std=std)
                if module.bias is not None:
                    module.bias.zero_()
            elif isinstance(module, Embedding):
                module.weight.normal_(mean=0.0, std=std)
            elif isinstance(module, Norm):
                module.weight.fill_(1.0)
                if module.bias is not None:
                    module.bias.zero_()
            elif getattr(module, "_mm_pretrained", False):
                pass                                                  # the MoE gate: built by its own from_pretrained, never re-initialised
            elif isinstance(module, XIELU):
                pass                                                  # Apertus: the activation's scalars keep HF's constructor values
            else:
                for n, p in module.named_parameters(recurse=False):   # class/position embeddings, patch conv
                    p.normal_(mean=0.0, std=std)

    def _component_params(self):
        """(name, parameter, component, weight_decay) for every parameter; weight_decay follows HF Trainer's grouping."""
        from ..nn import hf_decays
        owner = {}
        for mod in self.modules():
            for p in mod._parameters.values():
                if p is not None:
                    owner.setdefault(id(p), mod)
        seen, out = set(), []
        for n, p in self.model.named_parameters():
            if id(p) not in seen:
                seen.add(id(p))
                out.append(("model." + n, p, "llm", hf_decays("model." + n, owner.get(id(p)))))
        for i, m in enumerate(self.modalities_with_projection):
            # `train_gate` modalities: the gate is a component of its own.  HF's decay rule (hf_decays) decays BatchNorm weights
            # (`bn1.weight`, `downsample.1.weight`: neither nn.LayerNorm nor a name it excludes) and not the biases, as it
            # would for the reference's torchvision ResNet
            train_gate = bool(getattr(getattr(m, "config", None), "train_gate", False)) and isinstance(
                getattr(m, "gating_network", None), nn.Module)
            for n, p in m.named_parameters():
                gate = n.startswith("gating_network.")
                if id(p) in seen or (gate and not train_gate):           # the MoE gate is frozen by default: outside the flat
                    continue                                              # buffer, the gradient buckets and the optimiser
                seen.add(id(p))
                comp = f"gate{i}" if gate else (f"projector{i}" if n.startswith("projector.") else f"encoder{i}")
                full = f"modalities_with_projection.{i}.{n}"
                out.append((full, p, comp, hf_decays(full, owner.get(id(p)))))
        return out

    def pack_parameters(self) -> FlatParams:
        """Lay all parameters out in one flat buffer (fused q/k/v and gate/up operands, flat grads, flat AdamW)."""
        params = self._component_params()
        dtype = get_torch_dtype(self.config.dtype)
        dev = params[0][1].device
        self._flat = FlatParams(params, dev, dtype)
        return self._flat

    def flat_params(self) -> FlatParams:
        if self._flat is None:
            self.pack_parameters()
        return self._flat

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self._flat = None            # views into the old flat buffer are gone: re-pack lazily
        return out

    def _checkpoint_tensors(self):
        """What a checkpoint holds: every parameter, and the persistent buffers (the MoE gate's BatchNorm statistics, integer
        `num_batches_tracked` included: the reference's state dict carries them)."""
        own = dict(self.named_parameters())
        sd_keys = set(self.state_dict().keys())
        for k, b in self.named_buffers():
            if k in sd_keys and k not in own:
                own[k] = b
        return own

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        sd = dict(state_dict)
        self.model.drop_decode_weights()           # the MXFP8 decode copies are a snapshot of the weights being replaced
        own = self._checkpoint_tensors()
        # the reference keeps the whole CLIPModel; accept and ignore its unused towers / buffers
        unused = [k for k in sd if k not in own and any(t in k for t in ("text_model", "text_projection", "visual_projection",
                                                                         "logit_scale", "position_ids", "post_layernorm"))]
        for k in unused:
            sd.pop(k)
        if "model.lm_head.weight" in sd and self._llm_cfg.tie_word_embeddings:
            sd.pop("model.lm_head.weight")
        missing = [k for k in own if k not in sd]
        extra = [k for k in sd if k not in own]
        if strict and (missing or extra):
            raise RuntimeError(f"load_state_dict: missing={missing[:5]}... unexpected={extra[:5]}...")
        with torch.no_grad():
            for k, v in sd.items():
                if k in own:
                    own[k].copy_(v.to(device=own[k].device, dtype=own[k].dtype).reshape(own[k].shape))
        return missing, extra

    # known-ignorable keys of a reference checkpoint: the reference keeps the whole CLIPModel (text tower, projections,
    # logit_scale: SURVEY Appendix B) and HF buffers; a tied lm_head is stored under both names
    _IGNORABLE = ("text_model", "text_projection", "visual_projection", "logit_scale", "position_ids", "post_layernorm",
                  "rotary_emb.inv_freq")

    def save_pretrained(self, path: str, max_shard_size: int = 5 * 1024 ** 3, safe_serialization: bool = True):
        """HF layout (reference model.py:152-202 config + `PreTrainedModel.save_pretrained` weights): config.json with
        `MultimodalConfig.to_dict`, and the weights under the reference's parameter names as `model.safetensors`, or as
        `model-0000i-of-0000N.safetensors` + `model.safetensors.index.json` when they exceed `max_shard_size` (what an 8B
        checkpoint looks like).  Waits for in-flight device work first (the trainer's AdamW runs on a side stream)."""
        from safetensors.torch import save_file
        os.makedirs(path, exist_ok=True)
        self.config.save_pretrained(path)
        try:                                       # the LLM shape travels with the checkpoint only when llm_path cannot name it
            resolve_llm_config(self.config.llm_path)
        except (ValueError, OSError):
            with open(os.path.join(path, "llm_config.json"), "w") as f:
                json.dump(self._llm_cfg.to_dict(), f, indent=2)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        names = list(self._checkpoint_tensors().items())
        shards, cur, cur_bytes = [], [], 0
        for k, v in names:
            nb = v.numel() * v.element_size()
            if cur and cur_bytes + nb > max_shard_size:
                shards.append(cur)
                cur, cur_bytes = [], 0
            cur.append((k, v))
            cur_bytes += nb
        if cur:
            shards.append(cur)
        if len(shards) == 1:
            save_file({k: v.detach().cpu().contiguous().clone() for k, v in shards[0]}, os.path.join(path, "model.safetensors"),
                      metadata={"format": "pt"})
            return
        weight_map, total = {}, 0
        for i, sh in enumerate(shards):
            fn = f"model-{i + 1:05d}-of-{len(shards):05d}.safetensors"
            save_file({k: v.detach().cpu().contiguous().clone() for k, v in sh}, os.path.join(path, fn), metadata={"format": "pt"})
            for k, v in sh:
                weight_map[k] = fn
                total += v.numel() * v.element_size()
        with open(os.path.join(path, "model.safetensors.index.json"), "w") as f:
            json.dump({"metadata": {"total_size": total}, "weight_map": weight_map}, f, indent=2, sort_keys=True)

    def load_checkpoint_weights(self, path: str, strict: bool = True):
        """Stream `model.safetensors` or the shards listed by `model.safetensors.index.json` into the parameters, tensor by
        tensor (no whole-checkpoint host copy).  -> (missing, unexpected); raises when strict and either is non-empty
        after the known-ignorable keys (CLIP text tower etc.) are set aside."""
        from safetensors import safe_open
        idx = os.path.join(path, "model.safetensors.index.json")
        if os.path.exists(idx):
            files = sorted(set(json.load(open(idx))["weight_map"].values()))
        elif os.path.exists(os.path.join(path, "model.safetensors")):
            files = ["model.safetensors"]
        else:
            raise FileNotFoundError(f"{path}: neither model.safetensors nor model.safetensors.index.json")
        self.model.drop_decode_weights()
        own = self._checkpoint_tensors()
        seen, unexpected = set(), []
        tied = self._llm_cfg.tie_word_embeddings
        with torch.no_grad():
            for fn in files:
                with safe_open(os.path.join(path, fn), framework="pt", device="cpu") as f:
                    for k in f.keys():
                        if k == "model.lm_head.weight" and tied:
                            continue
                        if k not in own:
                            if not any(t in k for t in self._IGNORABLE):
                                unexpected.append(k)
                            continue
                        p = own[k]
                        p.copy_(f.get_tensor(k).to(dtype=p.dtype).reshape(p.shape))
                        seen.add(k)
        missing = [k for k in own if k not in seen]
        if strict and (missing or unexpected):
            raise RuntimeError(f"{path}: missing keys {missing[:8]}{'...' if len(missing) > 8 else ''}; "
                               f"unexpected keys {unexpected[:8]}{'...' if len(unexpected) > 8 else ''}")
        if missing or unexpected:
            logger.warning(f"{path}: {len(missing)} missing / {len(unexpected)} unexpected keys (left at their initial values)")
        return missing, unexpected

    @classmethod
    def from_pretrained(cls, path: str, device=None, strict: bool = True, **kwargs):
        """`kwargs` override fields of the stored config, as HF's `from_pretrained(path, truncation=..., max_sequence_length=...)`
        does for the reference (cli/train.py:131-137)."""
        raw = json.load(open(os.path.join(path, "config.json")))

        def local(name):      # a relative model directory stored beside the checkpoint (the reference resolves it against the cwd)
            if isinstance(name, str) and not os.path.isabs(name) and not os.path.isdir(name) and os.path.isdir(os.path.join(path, name)):
                return os.path.join(path, name)
            return name

        raw["llm_path"] = local(raw.get("llm_path"))
        for m in raw.get("modalities", []):
            for key in ("clip_name", "image_processor"):
                if key in m:
                    m[key] = local(m[key])
            if "expert_clip_names" in m:
                m["expert_clip_names"] = [local(x) for x in m["expert_clip_names"]]
        cfg = MultimodalConfig.from_dict(raw, **{k: v for k, v in kwargs.items() if k in ("truncation", "max_sequence_length", "dtype")})
        llm_cfg = None
        p = os.path.join(path, "llm_config.json")
        if os.path.exists(p):
            llm_cfg = json.load(open(p))
        model = cls(cfg, device=device, llm_config=llm_cfg)
        model.load_checkpoint_weights(path, strict=strict)
        return model

    # ------------------------------------------------------------------ freeze policies (model.py:310-377)
    def freeze_for_alignment(self):
        for m in self.modalities_with_projection:
            m.unfreeze_projection()
            m.freeze_modality_embedder()
        for p in self.model.parameters():
            p.requires_grad = False

    def freeze_for_lm(self):
        for m in self.modalities_with_projection:
            m.freeze_all()
        for p in self.model.parameters():
            p.requires_grad = True

    def freeze_for_end2end(self):
        for m in self.modalities_with_projection:
            m.unfreeze_projection()
            m.freeze_modality_embedder()
        for p in self.model.parameters():
            p.requires_grad = True

    def unfreeze(self):
        for m in self.modalities_with_projection:
            m.unfreeze_all()
        for p in self.model.parameters():
            p.requires_grad = True

    # ------------------------------------------------------------------ accessors (model.py:379-408)
    def processors(self) -> Dict[str, BaseModalityProcessor]:
        return self.processors_by_type

    def get_model(self):
        return self.model

    def _get_modality_by_name(self, name: str) -> BaseModality:
        if name not in self.modalities_by_type:
            raise KeyError(f"No modality registered in the model that can handle modality named: {name}")
        modality = self.modalities_by_type[name]
        if not isinstance(modality, BaseModality):
            raise TypeError(f"Registered modality {name} is not of type ModalityWithProjection")
        return modality

    def get_input_embeddings(self):
        return self.model.get_input_embeddings()

    def set_input_embeddings(self, value):
        self.model.set_input_embeddings(value)

    @property
    def device(self):
        return self.model.device

    @property
    def dtype(self):
        return self.model.dtype

    # ------------------------------------------------------------------ the hot path
    def embed_modalities_with_text(self, input_ids: torch.Tensor, processed_multimodal_inputs, stages=None):
        """model.py:410-446 as ONE gather pass: out[b,s] = projected modality row if (b,s) is in
        (batch_idx, token_range) else embedding[input_ids[b,s]]."""
        if self._flat is None:
            self.pack_parameters()
        dev = self.device
        input_ids = input_ids.to(dev)
        B, S = input_ids.shape
        projs, bis, trs = [], [], []
        pmi = processed_multimodal_inputs or {}
        for name, stack in (pmi.get("stacked") or {}).items():
            if len(stack) == 0:
                continue
            modality = self._get_modality_by_name(name)
            with trace_range(f"modality:{name}"):
                e = modality(stack, stages=stages) if stages is not None else modality(stack)
            projs.append(e.reshape(-1, e.shape[-1]))
            bis.append(pmi["batch_idx"][name].to(dev))
            trs.append(pmi["token_range"][name].to(dev))
        proj = bi = tr = None
        if projs:
            proj = projs[0] if len(projs) == 1 else torch.cat(projs, dim=0)
            bi = (bis[0] if len(bis) == 1 else torch.cat(bis)).to(torch.int64).contiguous()
            tr = (trs[0] if len(trs) == 1 else torch.cat(trs)).to(torch.int64).contiguous()
        with trace_range("embed_splice"):
            out = self.model.get_input_embeddings()(input_ids, proj, bi, tr)    # through __call__: parameter-read hooks fire
        return out.view(B, S, -1)

    def forward(self, input_ids: torch.LongTensor = None, inputs_embeds: Optional[torch.Tensor] = None,
                attention_mask: Optional[torch.Tensor] = None, position_ids: Optional[torch.LongTensor] = None,
                past_key_values=None, labels: Optional[torch.LongTensor] = None, use_cache: Optional[bool] = None,
                multimodal_inputs=None, processed_multimodal_inputs=None, return_dict: Optional[bool] = True,
                cache_position=None, **kwargs) -> Union[tuple, CausalLMOutput]:
        if self._flat is None:
            self.pack_parameters()
        if inputs_embeds is None:
            inputs_embeds = self.embed_modalities_with_text(input_ids, processed_multimodal_inputs)
        msl = self.config.max_sequence_length
        if self.config.truncation and msl is not None and inputs_embeds.shape[1] > msl:
            logger.warning(f"Truncating input to {msl} tokens.")
            inputs_embeds = inputs_embeds[:, :msl, :]
            labels = labels[:, :msl] if labels is not None else None
            kwargs.pop("loss_rows", None)                    # built from the untruncated labels
            attention_mask = attention_mask[:, :msl] if attention_mask is not None else None
            position_ids = position_ids[:, :msl] if position_ids is not None else None
        with trace_range("decoder+loss"):
            return self.model(inputs_embeds=inputs_embeds, attention_mask=attention_mask, position_ids=position_ids,
                              past_key_values=past_key_values, use_cache=use_cache, labels=labels, return_dict=return_dict,
                              **kwargs)

    def generate(self, batch: Dict[str, Any], max_new_tokens=512, temperature=0.1, do_sample=True, sync_every: int = 16,
                 top_k: Optional[int] = None, top_p: Optional[float] = None, min_p: Optional[float] = None,
                 seed: Optional[int] = None, generator: Optional[torch.Generator] = None, decode_weights: Optional[str] = None,
                 kv_cache: Optional[str] = None, prefill_weights: Optional[str] = None, num_return_sequences: int = 1,
                 num_beams: int = 1, length_penalty: float = 1.0, early_stopping=False, return_beam_scores: bool = False,
                 repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                 min_new_tokens: Optional[int] = None, suppress_tokens: Optional[Sequence[int]] = None,
                 prompt_lookup_num_tokens: Optional[int] = None, max_matching_ngram_size: Optional[int] = None,
                 return_lookup_stats: bool = False, guidance_scale: Optional[float] = None,
                 negative_batch: Optional[Dict[str, Any]] = None, **kwargs) -> torch.Tensor:
        """model.py:528-640: KV-cache decode.  Token choice = argmax(softmax(logits/T)) (one kernel) or a per-row
        multinomial draw; decode position = padded prompt length + i - 1 for every row (reference quirk :582-586);
        rows that already emitted eos keep emitting eos; returns [B, n_new] int64 on CPU without the prompt.

        Sampling (do_sample=True) takes one of two paths:
          - none of top_k / top_p / min_p / seed / generator given: torch.softmax + torch.multinomial, the reference-compatible
            consumer of torch's global RNG (the same torch seed gives the reference's draws);
          - any of them given: the device sampler mm_sample (temperature -> top-k -> top-p -> min-p, HF warper order; contract in
            include/mm_hip.h), step i drawing with Philox offset i and call = row.  `seed` is used as given; without it one int64
            is drawn from `generator` (torch's default CPU generator when None), so torch.manual_seed still fixes the ids.
            top_k = 0, top_p = 1 and min_p = 0 switch a warper off.
        Whether the device sampler should become the default is a separate decision.

        decode_weights="mxfp8" (opt-in): the decode steps stream weight-only MXFP8 copies of the decoder's matrices and lm_head
        (CausalLM.quantize_decode_weights: about half the weight bytes per token, ~8.3 GB more HBM on the 8B model, and the
        quantisation's error in the logits); the prefill reads the bf16 weights.  The copies are made on first use and reused:
        they are a snapshot (train(), load_state_dict / from_pretrained and resize_token_embeddings drop it; after any other weight
        update call model.model.quantize_decode_weights() again).  A call that cannot use them -- a model that is not bf16, more than
        16 sequences, activation rows that do not fit the kernel's LDS stage -- raises ValueError before the prefill.

        kv_cache="mxfp8" (opt-in): the K and V rows of every cached position are kept as e4m3 elements with one power-of-two scale
        per 32 values of a head (include/mm_hip.h: mm_kv8_*): 132 bytes per head row against 256, so a cached position of the 8B
        geometry costs 66 KiB over its 32 layers instead of 128 KiB.  The prefill is NOT quantised: it attends over the bf16 keys and
        values of the prompt (its logits, hence the first token, are the bf16 cache's bit for bit) and stores them quantised; every
        later step reads quantised keys and values, the current token's included.  Composes with decode_weights and every
        sampler path.  A model that cannot use it -- not bf16, head_dim other than 128, a number of query heads per key/value
        head other than 1, 2 or 4 -- raises ValueError before the prefill (CausalLM.kv_cache_ok).

        prefill_weights="mxfp8" (opt-in): the PREFILL call runs its decoder-layer linears as MXFP8 x MXFP8 GEMMs on the block-scaled
        MFMA (include/mm_hip.h: mm_gemm_mx8) -- the same copies decode_weights reads (made on first use: the same ~8.3 GB of HBM on the 8B model, the same
        snapshot rule), and each linear's input quantised on the way in (CausalLM.forward).  Only the prefill: the decode steps are governed by decode_weights as before; the vision towers, the
        projector, the splice and lm_head stay bf16.  It adds the quantisation's error to the prompt's logits and cached keys /
        values.  Composes with decode_weights, kv_cache and every sampler path.  A model that cannot use it -- not bf16, a linear
        whose input width mm_gemm_mx8 refuses (not a multiple of 128) -- raises ValueError before the prefill
        (CausalLM.prefill_weights_ok).

        num_return_sequences=n > 1, repetition_penalty= / no_repeat_ngram_size= / min_new_tokens= / suppress_tokens=, num_beams=n > 1 and
        prompt_lookup_num_tokens=k (each opt-in): see decoding.Sampling, decoding.BeamSearch and decoding.PromptLookup, the strategies
        the one decode loop (_decode) runs for them.

        guidance_scale=s with negative_batch= (opt-in): classifier-free guidance in ONE decoder pass per token, transformers'
        guidance_scale / negative_prompt_ids (UnbatchedClassifierFreeGuidanceLogitsProcessor): scores = log_softmax(uncond) + s *
        (log_softmax(cond) - log_softmax(uncond)) replace the logits in front of the processors and the selection.  negative_batch is
        a collated batch of the same B rows (input_ids, attention_mask, position_ids, processed_multimodal_inputs; with modalities of
        its own or none, e.g. the same conversation without its image: contrastive decoding against the language prior); None gives
        HF's default, the last prompt id as one position.  s: a finite number, not a bool; None or 1.0 is off and nothing changes
        (negative_batch must then be None).  See decoding.Sampling for the rows, positions and what it does not compose with."""
        n = _int_arg("num_return_sequences", num_return_sequences, 1)
        nb = _int_arg("num_beams", num_beams, 1, 16)
        pk, mg = prompt_lookup_num_tokens, max_matching_ngram_size
        given = [k for k, v in (("top_k", top_k), ("top_p", top_p), ("min_p", min_p), ("seed", seed), ("generator", generator)) if v is not None]
        on = {"beams": nb > 1, "no beams": nb == 1, "lookup": pk is not None, "no lookup": pk is None, "samples": n > 1 and nb == 1,
              "return_beam_scores": bool(return_beam_scores), "lookup arguments": bool(return_lookup_stats) or mg is not None,
              "do_sample": bool(do_sample), "greedy": not do_sample, "sampler": bool(given), "sampling": bool(do_sample) or bool(given),
              "kv_cache": kv_cache is not None}
        val = dict(n=n, nb=nb, pk=pk, kv_cache=kv_cache, sampler=", ".join(given),
                   sampling=", ".join((["do_sample=True"] if do_sample else []) + given))
        _refuse(_REFUSALS[:1], on, val)          # as ever: this one before the processors' values are looked at, the others after
        processors = self._logits_processors(repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens)
        on["processors"] = processors is not None
        if processors is not None:
            val["processors"] = ", ".join(k for k, v in zip(("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "suppress_tokens"),
                                                            (processors[0] != 1.0, processors[1] > 0, processors[2] > 0, len(processors[3]) > 0)) if v)
        guided = guidance_scale is not None and float(_number_arg("guidance_scale", guidance_scale)) != 1.0
        if negative_batch is not None and not guided:
            raise ValueError(f"negative_batch needs guidance_scale (a finite number other than 1.0), got guidance_scale={guidance_scale!r}")
        on["guidance"], val["gs"] = guided, guidance_scale
        if guided and negative_batch is not None:
            missing = [k for k in ("input_ids", "attention_mask", "position_ids", "processed_multimodal_inputs") if k not in negative_batch]
            if missing:
                raise ValueError(f"negative_batch (guidance_scale={guidance_scale!r}) lacks {', '.join(missing)}: a collated batch is expected")
        if pk is not None:
            _int_arg("prompt_lookup_num_tokens", pk, 1)
            mg = _int_arg("max_matching_ngram_size", 2 if mg is None else mg, 1)
        _refuse(_REFUSALS[1:], on, val)
        opt_in = guided or pk is not None or nb > 1 or n > 1 or any(v is not None for v in (kv_cache, decode_weights, prefill_weights))
        B, Sp = (int(d) for d in batch["input_ids"].shape[:2]) if opt_in else (None, None)
        own = None                               # the mode's own entry of CausalLM.OPTIONS
        if pk is not None:
            if B * (pk + 1) > 16:
                raise ValueError(f"prompt_lookup_num_tokens={pk} on {B} sequences: B (k + 1) = {B * (pk + 1)} rows, a verify step takes at most 16")
            strategy, own = PromptLookup(pk, mg, temperature, bool(return_lookup_stats)), ("prompt_lookup_num_tokens", pk)
        elif nb > 1:
            if n > nb:
                raise ValueError(f"num_return_sequences={n} > num_beams={nb}")
            _number_arg("length_penalty", length_penalty)
            if not (early_stopping is False or early_stopping is True or (isinstance(early_stopping, str) and early_stopping == "never")):
                raise ValueError(f"early_stopping must be False, True or 'never', got {early_stopping!r}")
            strategy, own = BeamSearch(nb, n, float(length_penalty), early_stopping, return_beam_scores), ("num_beams", nb)
        else:
            strategy = Sampling(temperature, do_sample, None, n, kv_cache, processors,
                                (float(guidance_scale), negative_batch) if guided else None)
            if n > 1:
                own = ("num_return_sequences", n)
            if guided and negative_batch is not None and tuple(negative_batch["input_ids"].shape[:1]) != (B,):
                raise ValueError(f"negative_batch of {tuple(negative_batch['input_ids'].shape)[0]} rows with guidance_scale={guidance_scale!r} "
                                 f"on a batch of {B}: one unconditional row per row")
        if opt_in:                               # a call without opt-ins reads neither the batch nor the decoder before _decode
            llm = self.model
            if own is not None:
                llm.check_option(*own, B, own[1])
            llm.check_option("kv_cache", kv_cache, B)
            llm.check_option("decode_weights", decode_weights, strategy.rows(B))                  # the rows of a decode step
            llm.check_option("prefill_weights", prefill_weights, B, Sp, check_grad=False)         # the loop runs under no_grad
            if guided:                                                                            # the second prefill, at its own length
                llm.check_option("prefill_weights", prefill_weights, B, 1 if negative_batch is None else int(negative_batch["input_ids"].shape[1]),
                                 check_grad=False)
        if do_sample and given:
            strategy.sampler = _device_sampler(top_k, top_p, min_p, seed, generator)
        return self._decode(strategy, batch, max_new_tokens, sync_every, decode_weights, prefill_weights)

    def _logits_processors(self, repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens):
        """generate()'s four processor arguments, checked -> (p, g, min_new_tokens, suppressed ids), or None when all are off."""
        p = _number_arg("repetition_penalty", 1.0 if repetition_penalty is None else repetition_penalty, positive=True)
        g = _int_arg("no_repeat_ngram_size", 0 if no_repeat_ngram_size is None else no_repeat_ngram_size, 0)
        mn = _int_arg("min_new_tokens", 0 if min_new_tokens is None else min_new_tokens, 0)
        if suppress_tokens is not None and (isinstance(suppress_tokens, (str, bytes)) or not hasattr(suppress_tokens, "__iter__")):
            raise ValueError(f"suppress_tokens must be a sequence of ints, got {suppress_tokens!r}")
        sup = [] if suppress_tokens is None else list(suppress_tokens)
        if float(p) == 1.0 and g == 0 and mn == 0 and not sup:
            return None
        V = self._llm_cfg.vocab_size
        for t in sup:
            if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < V:
                raise ValueError(f"suppress_tokens must be ints in [0, {V}), got {t!r}")
        eos = self.config.eos_token_idx
        if mn > 0 and (isinstance(eos, bool) or not isinstance(eos, int) or not 0 <= eos < V):
            raise ValueError(f"min_new_tokens={mn} needs config.eos_token_idx in [0, {V}), got {eos!r}")
        return float(p), g, mn, sup

    def _decode(self, strategy, batch, max_new_tokens, sync_every, decode_weights=None, prefill_weights=None):
        """generate()'s one decode loop: the prefill and up to max_new_tokens - 1 further decoder passes, with what is chosen from
        their logits and what the next pass is fed left to `strategy` (decoding.py).  Everything between two passes stays on the
        device; the host looks at the strategy's done flag every sync_every passes -- the only synchronisation of the loop -- and
        passes issued after every row had finished change nothing that is returned."""
        if self._flat is None:
            self.pack_parameters()
        dev, llm = self.device, self.model
        input_ids = batch["input_ids"].to(dev)
        if max_new_tokens <= 0:
            ids, extra = strategy.empty(input_ids.shape[0])
            return (ids, extra) if strategy.returns_extra else ids
        if decode_weights is not None and llm._decode_w8 is None:
            llm.quantize_decode_weights(decode_weights)
        dw = {"decode_weights": decode_weights} if decode_weights is not None else {}
        pw = {"prefill_weights": prefill_weights} if prefill_weights is not None else {}      # the prefill call only
        with torch.no_grad():
            feed = dict(inputs_embeds=self.embed_modalities_with_text(input_ids, batch["processed_multimodal_inputs"]),
                        attention_mask=batch["attention_mask"].to(dev), position_ids=batch["position_ids"].to(dev), logits_to_keep=1)
            mask = feed["attention_mask"]
            Smax, kw = strategy.cache_args(mask.shape[1], max_new_tokens)
            cache = llm.new_cache(mask.shape[0], Smax, **kw)
            strategy.begin(self, cache, input_ids, mask, max_new_tokens)
            for i in range(max_new_tokens):
                logits = llm(past_key_values=cache, use_cache=True, **feed, **dw, **pw).logits
                second = strategy.second_prefill() if i == 0 else None
                if second is not None:
                    logits = (logits, llm(past_key_values=cache, use_cache=True, **second, **dw, **pw).logits)
                pw = {}
                strategy.consume(logits, i)
                if i + 1 == max_new_tokens:
                    break
                if (i + 1) % max(1, sync_every) == 0 and bool(strategy.done()):      # the only host sync of the loop
                    break
                feed = strategy.feed(i + 1)
            ids, extra = strategy.finish()
            K.embed_check_pending()          # the host has just synchronised: an out-of-range input id raises here (IndexError)
        if strategy.trim_eos:
            # the reference stops right after the first step at which every row has emitted eos
            done = (ids == self.config.eos_token_idx).to(torch.int8).cummax(dim=1).values.bool().all(dim=0)
            if bool(done.any()):
                ids = ids[:, : int(torch.nonzero(done)[0]) + 1]
        return (ids, extra) if strategy.returns_extra else ids


def _int_arg(name, v, lo, hi=None, rng=None):
    """generate()'s "int in range, not bool" check; -> v"""
    if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
        rng = rng or (f">= {lo}" if hi is None else f"in [{lo}, {hi}]")
        raise ValueError(f"{name} must be an int {rng}, got {v!r}")
    return v


def _number_arg(name, v, positive=False):
    """generate()'s "finite number" check; -> v"""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or (positive and not v > 0):
        raise ValueError(f"{name} must be a finite number{' > 0' if positive else ''}, got {v!r}")
    return v


# generate(): which option excludes which, first match raised -- (the option that is on, what it meets, the message over `val`)
_REFUSALS = (
    ("no beams", "return_beam_scores", "return_beam_scores needs num_beams > 1"),
    ("no lookup", "lookup arguments", "return_lookup_stats / max_matching_ngram_size need prompt_lookup_num_tokens"),
    ("lookup", "sampling", "prompt_lookup_num_tokens={pk} with {sampling}: the lookup is greedy only (speculative sampling is out of scope)"),
    ("lookup", "beams", "prompt_lookup_num_tokens={pk} with num_beams={nb}: out of scope"),
    ("lookup", "samples", "prompt_lookup_num_tokens={pk} with num_return_sequences={n}: out of scope"),
    ("lookup", "kv_cache", "prompt_lookup_num_tokens={pk} with kv_cache={kv_cache!r}: the prompt-lookup cache is bf16 only"),
    ("lookup", "processors", "prompt_lookup_num_tokens={pk} with logits processors: filtering the candidates through them is out of scope"),
    ("beams", "processors", "num_beams={nb} with {processors}: logits processors inside beam search are out of scope"),
    ("beams", "do_sample", "num_beams={nb} needs do_sample=False: beam sampling is out of scope"),
    ("beams", "sampler", "num_beams={nb} with {sampler}: beam search does not sample"),
    ("beams", "kv_cache", "num_beams={nb} with kv_cache={kv_cache!r}: the beam cache is bf16 only (an MXFP8 beam cache is out of scope)"),
    ("samples", "greedy", "num_return_sequences={n} needs do_sample=True: greedy decoding would return {n} identical rows"),
    ("samples", "kv_cache", "num_return_sequences={n} with kv_cache={kv_cache!r}: the shared-prefix cache is bf16 only (an MXFP8 "
                            "shared-prefix cache is out of scope)"),
    ("guidance", "beams", "guidance_scale={gs} with num_beams={nb}: guidance inside beam search is out of scope"),
    ("guidance", "samples", "guidance_scale={gs} with num_return_sequences={n}: guided samples over a shared prompt are out of scope"),
    ("guidance", "lookup", "guidance_scale={gs} with prompt_lookup_num_tokens={pk}: guided verify steps are out of scope"),
    ("guidance", "kv_cache", "guidance_scale={gs} with kv_cache={kv_cache!r}: the guided cache is bf16 only (the second prefill would be "
                             "a multi-token store into a filled MXFP8 cache)"),
)


def _refuse(rows, on, val):
    for a, b, message in rows:
        if on[a] and on[b]:
            raise ValueError(message.format(**val))


def _device_sampler(top_k, top_p, min_p, seed, generator):
    """generate()'s device-sampler arguments, checked -> (top_k, top_p, min_p, seed); a missing seed is drawn from `generator`."""
    top_k = _int_arg("top_k", 0 if top_k is None else top_k, 0)
    top_p = 1.0 if top_p is None else top_p
    min_p = 0.0 if min_p is None else min_p
    if not (isinstance(top_p, (int, float)) and 0.0 < float(top_p) <= 1.0):
        raise ValueError(f"top_p must be in (0, 1], got {top_p!r}")
    if not (isinstance(min_p, (int, float)) and 0.0 <= float(min_p) <= 1.0):
        raise ValueError(f"min_p must be in [0, 1], got {min_p!r}")
    if seed is not None:
        return top_k, top_p, min_p, _int_arg("seed", seed, 0, (1 << 64) - 1, "in [0, 2**64)")
    gdev = generator.device if generator is not None else "cpu"
    return top_k, top_p, min_p, int(torch.randint(0, 1 << 62, (1,), generator=generator, device=gdev).item())


def bootstrap(config, tokenizer, modalities_config):
    """reference model.py:643-671"""
    mc = MultimodalConfig(hidden_size=config["token_size"], vocab_size=len(tokenizer),
                          eos_token_idx=tokenizer.convert_tokens_to_ids(tokenizer.eos_token), modalities=modalities_config,
                          llm_path=config["base_llm"], truncation=config.get("truncation", False),
                          max_sequence_length=config.get("max_sequence_length", None))
    return MultiModalModelForCausalLM(mc, bootstrap=True)
