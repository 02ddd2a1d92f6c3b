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
                 return_lookup_stats: bool = False, **kwargs) -> torch.Tensor:
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

        num_return_sequences=n > 1 (opt-in; needs do_sample=True, greedy would return n equal rows): n sampled continuations of
        every prompt.  The modalities are encoded, spliced and prefilled ONCE per prompt, and the prompt's keys and values are
        stored once (LayerKVCacheShared: 2 Hkv D 2 (B Sp + B n max_new_tokens) bytes per layer instead of n copies of the prompt);
        the prefill's last-row logits are repeated n times and every later step runs B n rows, whose decode attention reads a
        prompt's keys once per 16 / (Hq / Hkv) samples (include/mm_hip.h: mm_attn_decode_shared -- the bits of the replicated
        batch's attention).  Returns [B n, n_new]: row b n + j is sample j of prompt b (HF's order).  The device sampler draws
        with Philox offset = step and call = row b n + j; the torch.multinomial path draws per row; eos bookkeeping, sync_every,
        the early stop and the padded-length position quirk apply per row.  Composes with decode_weights (B n <= 16) and
        prefill_weights.  NOT with kv_cache="mxfp8" (a shared-prefix MXFP8 cache is out of scope: ValueError).  A model that
        cannot use it -- not bf16, head_dim other than 128, a number of query heads per key/value head other than 1, 2 or 4 --
        raises ValueError before the prefill (CausalLM.samples_ok).  n = 1 is the path above, untouched.

        num_beams=n > 1 (opt-in; needs do_sample=False): beam search as transformers' generate(num_beams=n, do_sample=False,
        length_penalty=, early_stopping=) with one eos token and no logits processors; the rules are written out in
        include/mm_hip.h (mm_beam_step).  One prefill per prompt into a LayerKVCacheBeam (the prompt's keys once, as above), then
        B n rows per step; the selection over a prompt's n V continuations, the finished hypotheses and the stopping flags live on the
        device (mm_beam_step), and a beam continues another row's suffix through an int32 ancestor table instead of a reordered
        cache (mm_attn_decode_beam).  The host looks at the device's done flag every `sync_every` steps; steps issued past it change
        nothing.  early_stopping in {False, True, "never"} and length_penalty have HF's meaning; temperature is ignored.  Returns
        [B num_return_sequences, n_out] (num_return_sequences <= n, default 1): row b nrs + k is prompt b's k-th best finished
        hypothesis, eos included and filled with eos behind its end, n_out the longest returned one; with return_beam_scores=True
        (ids, scores), scores [B nrs] fp32 = sum of log-probabilities / length ** length_penalty, descending per prompt.
        Composes with decode_weights (B n <= 16) and prefill_weights.  ValueError before the modalities are encoded for: num_beams
        outside [1, 16], do_sample=True, any of top_k / top_p / min_p / seed / generator, kv_cache="mxfp8", num_return_sequences >
        num_beams, a length_penalty that is not finite, another early_stopping, a vocabulary below 2 n, and a model samples_ok
        refuses.  num_beams = 1 is the code above, untouched.

        repetition_penalty= / no_repeat_ngram_size= / min_new_tokens= / suppress_tokens= (opt-in, each on its own): transformers'
        RepetitionPenalty -> NoRepeatNGram -> MinNewTokensLength -> SuppressTokens logits processors, applied in that order to the
        fp32 scores of every step by ONE kernel (include/mm_hip.h: mm_logits_process) between lm_head and the selection; greedy,
        torch.multinomial and the device sampler then select from its fp32 output unchanged.  The history of a row -- what the
        penalty and the n-gram ban look at -- lives on the device: the prompt's ids first, then every emitted id (the eos ids a
        finished row keeps emitting included), appended by the kernel; the host sees no token.  As in transformers' decoder-only
        generate the PROMPT counts, placeholder ids of spliced modalities like any id; the one deviation: positions whose
        attention_mask is 0 (pads) do not count (a pad == eos tokenizer would otherwise penalise eos on every padded row).
        repetition_penalty: a finite number > 0 (None or 1.0: off); no_repeat_ngram_size, min_new_tokens: ints >= 0 (None or 0: off;
        min_new_tokens bans config.eos_token_idx while step < min_new_tokens); suppress_tokens: ids in [0, vocab_size) that are never
        chosen, e.g. the attachment placeholder and pad ids (None or empty: off).  Compose with decode_weights, kv_cache,
        prefill_weights, num_return_sequences (every sample row keeps its own history) and every sampler path.  NOT with num_beams > 1
        (processors inside beam search act on log-probabilities inside mm_beam_step: out of scope, ValueError).  A bad value raises
        ValueError before the modalities are encoded.  With all four off nothing changes: no launch, no buffer, the same ids.

        prompt_lookup_num_tokens=k (opt-in; greedy: needs do_sample=False): prompt-lookup speculative decoding, transformers'
        generate(prompt_lookup_num_tokens=k, max_matching_ngram_size=G) for B rows at once.  Each iteration proposes up to k next
        tokens per row by matching the row's last n-gram (n <= G, default 2; the first match of the longest n) in its own visible
        prompt and output (include/mm_hip.h: mm_lookup_draft -- PromptLookupCandidateGenerator.get_candidates per row), runs ONE
        decoder pass over k + 1 positions per row -- B (k + 1) <= 16 rows, the rows a weight-streaming launch has to spare -- and keeps
        every proposed token the model would have chosen itself (mm_lookup_accept), so the ids are plain greedy decoding's up to the
        rounding of a differently sliced attention sum.  Rows advance by different amounts; their positions, histories and the done
        flag live on the device and the host reads only that flag, every `sync_every` iterations.  As everywhere here the prompt's
        masked positions do not count as history.  Returns the ids as above; with return_lookup_stats=True (ids, stats), stats int32
        [B, 2] on the CPU: verify steps run (the prefill's included) and draft tokens accepted, per row.  Composes with
        decode_weights (the verify step reads the copies) and prefill_weights.  Out of scope, ValueError before the modalities are
        encoded: sampling (do_sample=True, top_k / top_p / min_p / seed / generator), logits processors, num_beams > 1,
        num_return_sequences > 1 (shared-prefix samples), kv_cache="mxfp8", k not an int >= 1, B (k + 1) > 16, a model
        CausalLM.lookup_ok refuses, and return_lookup_stats / max_matching_ngram_size without k.  Not here either: a draft model
        (assistant_model), adaptive k, the append fused into the RoPE pass, tuned slice counts of the verify attention.  With
        prompt_lookup_num_tokens=None nothing changes: no launch, no buffer, the same ids."""
        n = num_return_sequences
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"num_return_sequences must be an int >= 1, got {n!r}")
        nb = num_beams
        if isinstance(nb, bool) or not isinstance(nb, int) or not 1 <= nb <= 16:
            raise ValueError(f"num_beams must be an int in [1, 16], got {nb!r}")
        if nb == 1 and return_beam_scores:
            raise ValueError("return_beam_scores needs num_beams > 1")
        processors = self._logits_processors(repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens)
        pk = prompt_lookup_num_tokens
        if pk is None:
            if return_lookup_stats or max_matching_ngram_size is not None:
                raise ValueError("return_lookup_stats / max_matching_ngram_size need prompt_lookup_num_tokens")
        else:
            if isinstance(pk, bool) or not isinstance(pk, int) or pk < 1:
                raise ValueError(f"prompt_lookup_num_tokens must be an int >= 1, got {pk!r}")
            mg = 2 if max_matching_ngram_size is None else max_matching_ngram_size
            if isinstance(mg, bool) or not isinstance(mg, int) or mg < 1:
                raise ValueError(f"max_matching_ngram_size must be an int >= 1, got {max_matching_ngram_size!r}")
            given = [a for a, v in (("top_k", top_k), ("top_p", top_p), ("min_p", min_p), ("seed", seed), ("generator", generator)) if v is not None]
            if do_sample or given:
                raise ValueError(f"prompt_lookup_num_tokens={pk} with {', '.join((['do_sample=True'] if do_sample else []) + given)}: the lookup "
                                 "is greedy only (speculative sampling is out of scope)")
            if nb > 1:
                raise ValueError(f"prompt_lookup_num_tokens={pk} with num_beams={nb}: out of scope")
            if n > 1:
                raise ValueError(f"prompt_lookup_num_tokens={pk} with num_return_sequences={n}: out of scope")
            if kv_cache is not None:
                raise ValueError(f"prompt_lookup_num_tokens={pk} with kv_cache={kv_cache!r}: the prompt-lookup cache is bf16 only")
            if processors is not None:
                raise ValueError(f"prompt_lookup_num_tokens={pk} with logits processors: filtering the candidates through them is out of scope")
            llm = self.model
            B, Sp = (int(d) for d in batch["input_ids"].shape[:2])
            if B * (pk + 1) > 16:
                raise ValueError(f"prompt_lookup_num_tokens={pk} on {B} sequences: B (k + 1) = {B * (pk + 1)} rows, a verify step takes at most 16")
            llm.check_option("prompt_lookup_num_tokens", pk, B, pk)
            llm.check_option("decode_weights", decode_weights, B * (pk + 1))                    # the verify steps run B (k + 1) rows
            llm.check_option("prefill_weights", prefill_weights, B, Sp, check_grad=False)
            return self._generate_lookup(batch, max_new_tokens, temperature, sync_every, pk, mg, bool(return_lookup_stats), decode_weights,
                                         prefill_weights)
        if nb > 1 and processors is not None:
            given = [k for k, on in zip(("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "suppress_tokens"),
                                        (processors[0] != 1.0, processors[1] > 0, processors[2] > 0, len(processors[3]) > 0)) if on]
            raise ValueError(f"num_beams={nb} with {', '.join(given)}: logits processors inside beam search are out of scope")
        if nb > 1:
            llm = self.model
            B, Sp = (int(d) for d in batch["input_ids"].shape[:2])
            if do_sample:
                raise ValueError(f"num_beams={nb} needs do_sample=False: beam sampling is out of scope")
            given = [k for k, v in (("top_k", top_k), ("top_p", top_p), ("min_p", min_p), ("seed", seed), ("generator", generator)) if v is not None]
            if given:
                raise ValueError(f"num_beams={nb} with {', '.join(given)}: beam search does not sample")
            if kv_cache is not None:
                raise ValueError(f"num_beams={nb} with kv_cache={kv_cache!r}: the beam cache is bf16 only (an MXFP8 beam cache is out of scope)")
            if n > nb:
                raise ValueError(f"num_return_sequences={n} > num_beams={nb}")
            if isinstance(length_penalty, bool) or not isinstance(length_penalty, (int, float)) or not math.isfinite(length_penalty):
                raise ValueError(f"length_penalty must be a finite number, got {length_penalty!r}")
            if not (early_stopping is False or early_stopping is True or (isinstance(early_stopping, str) and early_stopping == "never")):
                raise ValueError(f"early_stopping must be False, True or 'never', got {early_stopping!r}")
            llm.check_option("num_beams", nb, B, nb)
            llm.check_option("decode_weights", decode_weights, B * nb)                            # the decode steps run B n rows
            llm.check_option("prefill_weights", prefill_weights, B, Sp, check_grad=False)
            return self._generate_beams(batch, max_new_tokens, sync_every, nb, n, float(length_penalty), early_stopping,
                                        return_beam_scores, decode_weights, prefill_weights)
        if n > 1 or any(v is not None for v in (kv_cache, decode_weights, prefill_weights)):
            llm = self.model
            B, Sp = (int(d) for d in batch["input_ids"].shape[:2])
            if n > 1:
                if not do_sample:
                    raise ValueError(f"num_return_sequences={n} needs do_sample=True: greedy decoding would return {n} identical rows")
                if kv_cache is not None:
                    raise ValueError(f"num_return_sequences={n} with kv_cache={kv_cache!r}: the shared-prefix cache is bf16 only (an MXFP8 "
                                     "shared-prefix cache is out of scope)")
                llm.check_option("num_return_sequences", n, B, n)
            llm.check_option("kv_cache", kv_cache, B)
            llm.check_option("decode_weights", decode_weights, B * n)                             # the decode steps run B n rows
            llm.check_option("prefill_weights", prefill_weights, B, Sp, check_grad=False)         # the loop runs under no_grad
        device_sample = do_sample and any(a is not None for a in (top_k, top_p, min_p, seed, generator))
        if device_sample:
            top_k = 0 if top_k is None else top_k
            top_p = 1.0 if top_p is None else top_p
            min_p = 0.0 if min_p is None else min_p
            if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 0:
                raise ValueError(f"top_k must be an int >= 0, got {top_k!r}")
            if not (isinstance(top_p, (int, float)) and 0.0 < float(top_p) <= 1.0):
                raise ValueError(f"top_p must be in (0, 1], got {top_p!r}")
            if not (isinstance(min_p, (int, float)) and 0.0 <= float(min_p) <= 1.0):
                raise ValueError(f"min_p must be in [0, 1], got {min_p!r}")
            if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64):
                raise ValueError(f"seed must be an int in [0, 2**64), got {seed!r}")
            if seed is None:
                gdev = generator.device if generator is not None else "cpu"
                seed = int(torch.randint(0, 1 << 62, (1,), generator=generator, device=gdev).item())
        return self._generate(batch, max_new_tokens, temperature, do_sample, sync_every,
                              (top_k, top_p, min_p, seed) if device_sample else None, decode_weights, kv_cache, prefill_weights,
                              **({"samples": n} if n > 1 else {}), **({"processors": processors} if processors is not None else {}))

    def _logits_processors(self, repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens):
        """generate()'s four processor arguments, checked -> (p, g, min_new_tokens, suppressed ids), or None when all are off."""
        p = 1.0 if repetition_penalty is None else repetition_penalty
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not math.isfinite(p) or not p > 0:
            raise ValueError(f"repetition_penalty must be a finite number > 0, got {repetition_penalty!r}")
        g = 0 if no_repeat_ngram_size is None else no_repeat_ngram_size
        if isinstance(g, bool) or not isinstance(g, int) or g < 0:
            raise ValueError(f"no_repeat_ngram_size must be an int >= 0, got {no_repeat_ngram_size!r}")
        mn = 0 if min_new_tokens is None else min_new_tokens
        if isinstance(mn, bool) or not isinstance(mn, int) or mn < 0:
            raise ValueError(f"min_new_tokens must be an int >= 0, got {min_new_tokens!r}")
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

    def _generate(self, batch, max_new_tokens, temperature, do_sample, sync_every, sampler, decode_weights=None, kv_cache=None, prefill_weights=None,
                  samples: int = 1, processors=None) -> torch.Tensor:
        """generate()'s decode loop; sampler = (top_k, top_p, min_p, seed) for the device sampler, else None.

        The reference synchronises with the host after EVERY token (`.cpu()`, `finished.all()`, model.py:618-625,637-638).
        Here the chosen id, the eos bookkeeping and the next embedding lookup stay on the device (mm_decode_select +
        the embedding gather), so the host queues steps ahead of the GPU; it looks at `finished` only every `sync_every`
        tokens.  Steps issued past the point where every row had finished are cut off afterwards: the returned ids are
        exactly the reference's (same length, same values).

        samples = n > 1 (generate's num_return_sequences): the prefill runs on the B prompts into a LayerKVCacheShared; its logits
        are repeated n times and from there on B stands for the B n sample rows.  The decode steps hand the PROMPT's mask to the
        cache (generated tokens are always visible).

        processors = (repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppressed ids), checked by generate, else None: every
        step's logits go through mm_logits_process (one launch; the rows' history stays on the device, fed from next_ids) and the
        selection reads its fp32 output."""
        if self._flat is None:
            self.pack_parameters()
        dev = self.device
        input_ids = batch["input_ids"].to(dev)
        temperature = max(temperature, 1e-6)
        B = input_ids.shape[0]
        V = self._llm_cfg.vocab_size
        eos = self.config.eos_token_idx
        if max_new_tokens <= 0:
            return torch.empty((B * samples, 0), dtype=torch.int64)
        if decode_weights is not None and self.model._decode_w8 is None:
            self.model.quantize_decode_weights(decode_weights)
        dw = {"decode_weights": decode_weights} if decode_weights is not None else {}
        with torch.no_grad():
            nxt = self.embed_modalities_with_text(input_ids, batch["processed_multimodal_inputs"])
            attention_mask = batch["attention_mask"].to(dev)
            position_ids = batch["position_ids"].to(dev)
            seq_length = attention_mask.shape[1]
            if samples > 1:
                cache = self.model.new_cache(B, seq_length + max_new_tokens, samples=samples, prompt_len=seq_length)
                prompt_mask = attention_mask
                B = B * samples                                # the rows of every buffer below and of every step after the prefill
            else:
                cache = self.model.new_cache(B, seq_length + max_new_tokens, kv_cache=kv_cache)
            # device-resident loop state (plumbing): the growing mask is a view of one preallocated buffer
            if samples == 1:
                full_mask = torch.ones((B, seq_length + max_new_tokens), dtype=attention_mask.dtype, device=dev)
                full_mask[:, :seq_length] = attention_mask
            out_ids = torch.full((B, max_new_tokens), eos, dtype=torch.int64, device=dev)
            finished = torch.zeros(B, dtype=torch.uint8, device=dev)
            next_ids = torch.empty(B, dtype=torch.int64, device=dev)
            steps = 0
            emb = self.model.get_input_embeddings()
            sample_ws = K.sample_ws(B, V, dev) if sampler is not None else None       # once per call
            tok_buf = torch.empty(B, dtype=torch.int64, device=dev) if sampler is not None else None
            lp = None
            if processors is not None:
                p_, g_, mn_, sup_ = processors
                lp = K.LogitsState(B, V, dev, p_, g_, mn_, sup_, prompt_ids=input_ids, prompt_mask=batch["attention_mask"].to(dev),
                                   samples=samples, room=max_new_tokens)
            for i in range(max_new_tokens):
                if i > 0:
                    position_ids = torch.full((B, 1), seq_length + i - 1, dtype=torch.long, device=dev)
                    attention_mask = full_mask[:, : seq_length + i] if samples == 1 else prompt_mask
                pw = {"prefill_weights": prefill_weights} if i == 0 and prefill_weights is not None else {}      # the prefill call only
                out = self.model(inputs_embeds=nxt, attention_mask=attention_mask, position_ids=position_ids,
                                 past_key_values=cache, use_cache=True, logits_to_keep=1, **dw, **pw)
                logits2d = out.logits[:, -1, :]                       # [B, V] view, stride padded
                if samples > 1 and i == 0:
                    logits2d = logits2d.repeat_interleave(samples, dim=0)      # plumbing: sample j of prompt b is row b n + j
                if lp is not None:
                    logits2d = K.logits_process(logits2d, lp, i, next_ids, eos)    # fp32 scores; the history takes next_ids in
                if sampler is not None:
                    k_, p_, mp_, sd_ = sampler
                    tok = K.sample(logits2d, V, temperature, top_k=k_, top_p=p_, min_p=mp_, seed=sd_, offset=i, ws=sample_ws,
                                   out=tok_buf)
                elif do_sample:
                    probs = torch.softmax(logits2d.float() / temperature, dim=-1)
                    tok = torch.multinomial(probs, num_samples=1).view(B)
                else:
                    tok = K.argmax_softmax(logits2d, V, temperature)
                K.decode_select(tok, finished, eos, out_ids, i, next_ids)
                steps = i + 1
                if steps == max_new_tokens:
                    break
                if steps % max(1, sync_every) == 0 and bool(finished.all()):      # the only host sync of the loop
                    break
                nxt = emb(next_ids.view(B, 1))
            ids = out_ids[:, :steps].cpu()
            K.embed_check_pending()          # the host has just synchronised: an out-of-range input id raises here (IndexError)
        # the reference stops right after the first step at which every row has emitted eos
        done = (ids == eos).to(torch.int8).cummax(dim=1).values.bool().all(dim=0)
        if bool(done.any()):
            ids = ids[:, : int(torch.nonzero(done)[0]) + 1]
        return ids


    def _generate_beams(self, batch, max_new_tokens, sync_every, n, nrs, length_penalty, early_stopping, return_scores,
                        decode_weights=None, prefill_weights=None):
        """generate()'s beam-search loop (num_beams = n > 1, checked by generate).  The prefill runs on the B prompts into a
        LayerKVCacheBeam; mm_beam_step reads its B rows of logits at step 0 and B n rows afterwards, and hands back the next ids
        (the next embedding lookup) and the ancestor table of the coming step.  Nothing but the done flag comes to the host, every
        sync_every steps; positions keep the padded-length quirk of _generate and the cache gets the PROMPT's mask."""
        if self._flat is None:
            self.pack_parameters()
        dev = self.device
        input_ids = batch["input_ids"].to(dev)
        B = input_ids.shape[0]
        V = self._llm_cfg.vocab_size
        eos = self.config.eos_token_idx
        if max_new_tokens <= 0:
            ids = torch.empty((B * nrs, 0), dtype=torch.int64)
            return (ids, torch.zeros(B * nrs, dtype=torch.float32)) if return_scores else ids
        if decode_weights is not None and self.model._decode_w8 is None:
            self.model.quantize_decode_weights(decode_weights)
        dw = {"decode_weights": decode_weights} if decode_weights is not None else {}
        R = B * n
        with torch.no_grad():
            nxt = self.embed_modalities_with_text(input_ids, batch["processed_multimodal_inputs"])
            attention_mask = prompt_mask = batch["attention_mask"].to(dev)
            position_ids = batch["position_ids"].to(dev)
            seq_length = attention_mask.shape[1]
            cache = self.model.new_cache(B, seq_length + max_new_tokens, beams=n, prompt_len=seq_length)
            tables = cache[0].tables
            st = K.BeamState(B, n, max_new_tokens, V, dev)
            emb = self.model.get_input_embeddings()
            for i in range(max_new_tokens):
                if i > 0:
                    position_ids = torch.full((R, 1), seq_length + i - 1, dtype=torch.long, device=dev)
                    attention_mask = prompt_mask
                    tables.current = st.table(i)
                pw = {"prefill_weights": prefill_weights} if i == 0 and prefill_weights is not None else {}      # the prefill call only
                out = self.model(inputs_embeds=nxt, attention_mask=attention_mask, position_ids=position_ids,
                                 past_key_values=cache, use_cache=True, logits_to_keep=1, **dw, **pw)
                next_ids = K.beam_step(out.logits[:, -1, :], st, i, eos, length_penalty, early_stopping)
                if i + 1 == max_new_tokens:
                    break
                if (i + 1) % max(1, sync_every) == 0 and bool(st.done.item()):      # the only host sync of the loop
                    break
                nxt = emb(next_ids.view(R, 1))
            ids, scores, lens = K.beam_finish(st, nrs, eos)
            n_out = int(lens.max().item())
            ids, scores = ids[:, :n_out].cpu(), scores.cpu()
            K.embed_check_pending()          # the host has just synchronised: an out-of-range input id raises here (IndexError)
        return (ids, scores) if return_scores else ids


    def _generate_lookup(self, batch, max_new_tokens, temperature, sync_every, k, G, return_stats, decode_weights=None, prefill_weights=None):
        """generate()'s prompt-lookup loop (prompt_lookup_num_tokens = k, max_matching_ngram_size = G, checked by generate).  The
        prefill runs as in _generate into a LayerKVCacheLookup with room for k slots behind the last id; its token goes through
        mm_lookup_accept as a verify step without drafts, so count, finished, the history and base (seq_length - 1 -> seq_length: the
        "padded prompt length + i - 1" position and cache slot of the first generated token) start out the way later steps update
        them.  An iteration is mm_lookup_draft -> embedding gather -> one decoder pass over k + 1 positions per row (CausalLM.forward's
        "verify" route) with lm_head on all B (k + 1) rows -> the selector plain greedy uses, at the caller's temperature ->
        mm_lookup_accept.  At most max_new_tokens accept calls (every one emits at least one id per active row); the host reads the
        device's done flag every sync_every of them, and iterations issued after done change nothing."""
        if self._flat is None:
            self.pack_parameters()
        dev = self.device
        input_ids = batch["input_ids"].to(dev)
        temperature = max(temperature, 1e-6)
        B = input_ids.shape[0]
        V = self._llm_cfg.vocab_size
        eos = self.config.eos_token_idx
        if max_new_tokens <= 0:
            ids = torch.empty((B, 0), dtype=torch.int64)
            return (ids, torch.zeros((B, 2), dtype=torch.int32)) if return_stats else ids
        if decode_weights is not None and self.model._decode_w8 is None:
            self.model.quantize_decode_weights(decode_weights)
        dw = {"decode_weights": decode_weights} if decode_weights is not None else {}
        pw = {"prefill_weights": prefill_weights} if prefill_weights is not None else {}
        Q = k + 1
        with torch.no_grad():
            nxt = self.embed_modalities_with_text(input_ids, batch["processed_multimodal_inputs"])
            attention_mask = batch["attention_mask"].to(dev)
            position_ids = batch["position_ids"].to(dev)
            seq_length = attention_mask.shape[1]
            cache = self.model.new_cache(B, seq_length + max_new_tokens + k, lookup=k)
            st = K.LookupState(input_ids, attention_mask, k, G, max_new_tokens, eos, seq_length - 1)
            shared = cache[0].shared
            shared.base = st.base
            emb = self.model.get_input_embeddings()
            out = self.model(inputs_embeds=nxt, attention_mask=attention_mask, position_ids=position_ids, past_key_values=cache,
                             use_cache=True, logits_to_keep=1, **dw, **pw)
            K.lookup_accept(st, K.argmax_softmax(out.logits[:, -1, :], V, temperature), 1)
            prompt_mask = attention_mask.to(torch.int64).contiguous()
            for it in range(1, max_new_tokens):
                if it % max(1, sync_every) == 0 and bool(st.done.item()):      # the only host sync of the loop
                    break
                shared.bound = min(seq_length + (it - 1) * Q, seq_length + max_new_tokens - 1)      # base[b] <= bound, known here
                ids, pos = K.lookup_draft(st)
                out = self.model(inputs_embeds=emb(ids), attention_mask=prompt_mask, position_ids=pos, past_key_values=cache,
                                 use_cache=True, **dw)
                K.lookup_accept(st, K.argmax_softmax(out.logits.reshape(B * Q, V), V, temperature))
            ids, stats, count = st.out.cpu(), st.stats.cpu(), st.count.cpu()
            K.embed_check_pending()          # the host has just synchronised: an out-of-range input id raises here (IndexError)
        ids = ids[:, : int(count.max())]
        # the reference stops right after the first step at which every row has emitted eos
        done = (ids == eos).to(torch.int8).cummax(dim=1).values.bool().all(dim=0)
        if bool(done.any()):
            ids = ids[:, : int(torch.nonzero(done)[0]) + 1]
        return (ids, stats) if return_stats else ids


def bootstrap(config, tokenizer, modalities_config):
    """reference model.py:643-671"""
    mc = MultimodalConfig(hidden_size=config["token_size"], vocab_size=len(tokenizer),
                          eos_token_idx=tokenizer.convert_tokens_to_ids(tokenizer.eos_token), modalities=modalities_config,
                          llm_path=config["base_llm"], truncation=config.get("truncation", False),
                          max_sequence_length=config.get("max_sequence_length", None))
    return MultiModalModelForCausalLM(mc, bootstrap=True)
