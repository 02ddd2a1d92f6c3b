"""Apertus decoders (CPU): the config mapping, HF's parameter and buffer names (strict load of the fixture the REAL reference wrote),
the weight-decay flags, the Apertus-8B preset, the refused configuration, the saved configs of the other families (byte-identical to
what they were before `hidden_act` existed), the reference's alignment recipe with `tokenizer_type: apertus`, and a save -> reload
round trip.  No kernel runs here."""
import json
import os

import pytest
import torch

from multimeditron_amd.model.llm import LLMConfig
from multimeditron_amd.model.presets import LLM_PRESETS, resolve_llm_config
from tests.apertus_fixture import FIXTURES, load_apertus_golden
from tests.model_utils import build_from_golden

EPS_BF16 = -9.98377799987793e-07          # bf16(-1e-6)
# LLMConfig.to_dict() of a Llama / Qwen2 / Qwen3 config: the keys, in order, that the parent commit wrote (llm_config.json)
PARENT_KEYS = ["model_type", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "num_key_value_heads", "head_dim",
               "vocab_size", "rms_norm_eps", "tie_word_embeddings", "attention_bias", "qk_norm", "max_position_embeddings", "rope_parameters"]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_config_sets_qk_norm_and_xielu(golden_dir, name):
    meta, _, _ = load_apertus_golden(name, golden_dir)
    cfg = LLMConfig.from_dict(meta["llm"])
    assert cfg.model_type == "apertus" and cfg.apertus and cfg.qk_norm and cfg.hidden_act == "xielu" and not cfg.attention_bias
    assert cfg.head_dim == 128 and not cfg.tie_word_embeddings and cfg.pad_token_id == 3       # ApertusConfig's padding row
    assert cfg.rope_parameters["rope_type"] == "llama3" and cfg.rope_parameters["rope_theta"] == 12000000.0
    d = cfg.to_dict()
    assert d["hidden_act"] == "xielu" and LLMConfig.from_dict(d) == cfg
    other = LLMConfig.from_dict(dict(meta["llm"], model_type="llama"))
    assert not other.qk_norm and other.hidden_act == "silu" and other.pad_token_id is None


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_loads_strict_with_hf_names(golden_dir, tmp_path, name):
    meta, w, _ = load_apertus_golden(name, golden_dir)
    m = build_from_golden(meta, w, tmp_path, "float32", device="cpu")       # load_state_dict(strict=True)
    own = dict(m.named_parameters())
    bufs = {k: b for k, b in m.named_buffers() if k in m.state_dict()}
    assert set(own) | set(bufs) == set(w)
    for k, t in w.items():
        got = own[k] if k in own else bufs[k]
        assert got.shape == t.shape and torch.equal(got.detach(), t.float()), k
    for i in range(meta["llm"]["num_hidden_layers"]):
        p = f"model.model.layers.{i}."
        names = {k[len(p):] for k in list(own) + list(bufs) if k.startswith(p)}
        assert names == {"self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.o_proj.weight",
                         "self_attn.q_norm.weight", "self_attn.k_norm.weight", "mlp.up_proj.weight", "mlp.down_proj.weight",
                         "mlp.act_fn.alpha_p", "mlp.act_fn.alpha_n", "mlp.act_fn.beta", "mlp.act_fn.eps",
                         "attention_layernorm.weight", "feedforward_layernorm.weight"}
        f = m.model.model.layers[i].mlp.act_fn
        assert isinstance(f.alpha_p, torch.nn.Parameter) and f.alpha_p.shape == (1,) and f.alpha_n.shape == (1,)
        assert p + "mlp.act_fn.beta" in bufs and f.beta.shape == () and f.eps.shape == ()
        assert f.consts() == (0.5, EPS_BF16)
    a0, a1 = (m.model.model.layers[i].mlp.act_fn for i in (0, 1))
    assert tuple(float(t.detach()) for t in (a0.alpha_p, a0.alpha_n, a1.alpha_p, a1.alpha_n)) == (1.0, 0.5, -0.5, 1.5)


def test_new_model_has_hf_initial_scalars_and_rounded_eps(golden_dir, tmp_path):
    meta, w, _ = load_apertus_golden("tiny_clip_apertus", golden_dir)
    for dtype, tdt in (("bfloat16", torch.bfloat16), ("float32", torch.float32)):
        m = build_from_golden(meta, {k: v for k, v in w.items()}, tmp_path / dtype, dtype, device="cpu")
        from multimeditron_amd.model.llm import XIELU
        f = XIELU(tdt, "cpu")
        assert f.alpha_p.dtype == tdt and f.beta.dtype == tdt
        assert float(f.alpha_p.detach()) == float(torch.log(torch.expm1(torch.tensor(0.8, dtype=tdt))))      # HF computes them in the dtype
        assert float(f.alpha_n.detach()) == float(torch.log(torch.expm1(torch.tensor(0.8 - 0.5, dtype=tdt))))
        assert f.consts() == (0.5, float(torch.tensor(-1e-6, dtype=tdt)))
        assert m.model.model.layers[0].mlp.act_fn.alpha_p.dtype == tdt


def test_decay_flags_follow_hf(golden_dir, tmp_path):
    """HF Trainer's rule: `mlp.act_fn.alpha_p` / `alpha_n` match none of its exclusions and ARE decayed; the four norms are not."""
    from multimeditron_amd.nn import hf_decays
    meta, w, _ = load_apertus_golden("tiny_clip_apertus", golden_dir)
    m = build_from_golden(meta, w, tmp_path, "float32", device="cpu")
    owners = dict(m.named_modules())
    alphas = norms = 0
    for n, _p in m.named_parameters():
        owner = owners[n.rsplit(".", 1)[0]]
        if n.endswith(("act_fn.alpha_p", "act_fn.alpha_n")):
            assert hf_decays(n, owner), n
            alphas += 1
        elif n.endswith(("q_norm.weight", "k_norm.weight", "attention_layernorm.weight", "feedforward_layernorm.weight")):
            assert not hf_decays(n, owner), n
            norms += 1
    L = meta["llm"]["num_hidden_layers"]
    assert alphas == 2 * L and norms == 4 * L
    decay = {seg.name: seg.decay for seg in m.flat_params().segments}
    assert decay["model.model.layers.0.mlp.act_fn.alpha_p"] and not decay["model.model.layers.0.feedforward_layernorm.weight"]


def test_apertus_8b_preset():
    d = resolve_llm_config("swiss-ai/Apertus-8B-Instruct-2509")
    cfg = LLMConfig.from_dict(d)
    assert cfg.model_type == "apertus" and cfg.qk_norm and cfg.hidden_act == "xielu" and not cfg.attention_bias
    assert (cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers) == (4096, 21504, 32)
    assert (cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim, cfg.vocab_size) == (32, 8, 128, 131072)
    assert cfg.rms_norm_eps == 1e-5 and not cfg.tie_word_embeddings and cfg.max_position_embeddings == 65536
    assert cfg.rope_parameters == {"rope_type": "llama3", "rope_theta": 12000000.0, "factor": 8.0, "low_freq_factor": 1.0,
                                   "high_freq_factor": 4.0, "original_max_position_embeddings": 8192}
    assert LLM_PRESETS["swiss-ai/Apertus-8B-2509"] is LLM_PRESETS["swiss-ai/Apertus-8B-Instruct-2509"]


def test_apertus_with_another_activation_raises(golden_dir):
    meta, _, _ = load_apertus_golden("tiny_clip_apertus", golden_dir)
    with pytest.raises(NotImplementedError):
        LLMConfig.from_dict(dict(meta["llm"], hidden_act="silu"))
    with pytest.raises(NotImplementedError):
        LLMConfig.from_dict({"model_type": "apertus", "hidden_act": "silu"})
    assert LLMConfig.from_dict({"model_type": "apertus"}).hidden_act == "xielu"


@pytest.mark.parametrize("name, expect", [
    ("meta-llama/Llama-3.1-8B-Instruct", dict(model_type="llama", attention_bias=False, qk_norm=False, max_position_embeddings=131072)),
    ("Qwen/Qwen2-7B-Instruct", dict(model_type="qwen2", attention_bias=True, qk_norm=False, max_position_embeddings=131072)),
    ("Qwen/Qwen3-4B-Instruct-2507", dict(model_type="qwen3", attention_bias=False, qk_norm=True, max_position_embeddings=262144)),
])
def test_saved_config_of_other_families_is_unchanged(name, expect):
    """`llm_config.json` of a Llama / Qwen2 / Qwen3 model: exactly the parent commit's keys in its order, no `hidden_act`"""
    preset = resolve_llm_config(name)
    d = LLMConfig.from_dict(dict(preset, hidden_act="silu")).to_dict()      # HF config.json files carry hidden_act = silu
    assert list(d) == PARENT_KEYS
    want = {k: preset.get(k) for k in PARENT_KEYS}
    want.update(expect)
    assert json.dumps(d, indent=2) == json.dumps({k: want[k] for k in PARENT_KEYS}, indent=2)
    assert LLMConfig.from_dict(preset).to_dict() == d


def _apertus_dir(tmp_path):
    from tests.test_training_config_cpu import tiny_dirs
    llm, clips = tiny_dirs(tmp_path)
    cfg = json.load(open(os.path.join(llm, "config.json")))
    cfg.update(model_type="apertus", hidden_act="xielu", qk_norm=True,
               rope_parameters={"rope_type": "llama3", "rope_theta": 12000000.0, "factor": 8.0, "low_freq_factor": 1.0,
                                "high_freq_factor": 4.0, "original_max_position_embeddings": 8192})
    json.dump(cfg, open(os.path.join(llm, "config.json"), "w"))
    return llm, clips


def test_apertus_recipe_builds_model_collator_trainer(tmp_path):
    """The keys of the reference's alignment recipe with `tokenizer_type: apertus`; the LLM is a tiny local Apertus directory."""
    from tests.test_training_config_cpu import ATTACH, alignment_recipe, make_tokenizer
    from multimeditron_amd.train import from_training_config
    from multimeditron_amd.train.trainer import TrainingMode
    llm, clips = _apertus_dir(tmp_path)
    recipe = alignment_recipe(llm, clips[0])
    recipe.update(tokenizer_type="apertus", token_size=64)
    setup = from_training_config(recipe, make_tokenizer(), train_dataset=[{"text": "a cat ."}] * 64, device="cpu", dtype="float32")
    model, coll, tr = setup.model, setup.collator, setup.trainer
    llm_cfg = model.model.config
    assert llm_cfg.model_type == "apertus" and llm_cfg.qk_norm and llm_cfg.hidden_act == "xielu"
    layer = model.model.model.layers[0]
    assert layer.self_attn.q_norm is not None and hasattr(layer, "attention_layernorm") and hasattr(layer, "feedforward_layernorm")
    assert not hasattr(layer, "input_layernorm") and not hasattr(layer.mlp, "gate_proj")
    assert layer.mlp.act_fn.alpha_p.shape == (1,) and model.model.model.embed_tokens.padding_idx == 3
    assert coll.chat_template.name == "apertus" and coll.attachment_token == ATTACH
    assert tr.training_mode == TrainingMode.ALIGNMENT
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    assert trainable and all(".projector." in n for n in trainable)


def test_save_reload_roundtrip_cpu(golden_dir, tmp_path):
    from multimeditron_amd.model.model import MultiModalModelForCausalLM
    meta, w, _ = load_apertus_golden("tiny_clip_apertus", golden_dir)
    m = build_from_golden(meta, w, tmp_path / "a", "bfloat16", device="cpu")
    m.save_pretrained(str(tmp_path / "ckpt"))
    saved = json.load(open(tmp_path / "ckpt" / "llm_config.json"))
    assert saved["model_type"] == "apertus" and saved["hidden_act"] == "xielu"
    m2 = MultiModalModelForCausalLM.from_pretrained(str(tmp_path / "ckpt"), device="cpu")          # strict
    a, b = m._checkpoint_tensors(), m2._checkpoint_tensors()
    assert set(a) == set(b) and "model.model.layers.1.mlp.act_fn.eps" in a
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    assert float(m2.model.model.layers[1].mlp.act_fn.alpha_n.detach()) == 1.5
    assert m2.model.model.layers[0].mlp.act_fn.consts() == (0.5, EPS_BF16)
