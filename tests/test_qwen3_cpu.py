"""Qwen3 decoders (CPU): the config flag, the parameter names of the per-head q/k norms (strict load of the fixture the REAL
reference wrote), their weight-decay flag, the Qwen3-4B preset, the configurations that are refused, and the reference's Qwen
recipe (cookbook/sft/single_clip/two_phase_alignment/config_alignment_generalist_qwen.yaml) through from_training_config.
No kernel runs here."""
import json
import os

import pytest
import torch

from multimeditron_amd.model.llm import LLMConfig
from multimeditron_amd.model.presets import resolve_llm_config
from tests.qwen3_fixture import FIXTURES, load_qwen3_golden
from tests.model_utils import build_from_golden


def _tied(meta, k):
    return k == "model.lm_head.weight" and meta["llm"].get("tie_word_embeddings")


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_config_sets_qk_norm(golden_dir, name):
    meta, _, _ = load_qwen3_golden(name, golden_dir)
    cfg = LLMConfig.from_dict(meta["llm"])
    assert cfg.model_type == "qwen3" and cfg.qk_norm and not cfg.attention_bias
    assert cfg.head_dim == 128 and cfg.tie_word_embeddings
    assert not LLMConfig.from_dict(dict(meta["llm"], model_type="llama")).qk_norm


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_loads_strict_with_hf_names(golden_dir, tmp_path, name):
    meta, w, _ = load_qwen3_golden(name, golden_dir)
    m = build_from_golden(meta, w, tmp_path, "float32", device="cpu")       # load_state_dict(strict=True)
    own = dict(m.named_parameters())
    assert set(own) == {k for k in w if not _tied(meta, k)}
    for k, t in w.items():
        if not _tied(meta, k):
            assert torch.equal(own[k].detach(), t.float()), k
    for i in range(meta["llm"]["num_hidden_layers"]):
        a = m.model.model.layers[i].self_attn
        assert a.q_norm.weight.shape == (128,) and a.k_norm.weight.shape == (128,)
        assert f"model.model.layers.{i}.self_attn.q_norm.weight" in own and f"model.model.layers.{i}.self_attn.k_norm.weight" in own


def test_qk_norm_weights_are_not_decayed(golden_dir, tmp_path):
    from multimeditron_amd.nn import hf_decays
    meta, w, _ = load_qwen3_golden("tiny_clip_qwen3", golden_dir)
    m = build_from_golden(meta, w, tmp_path, "float32", device="cpu")
    owners = {n: mod for n, mod in m.named_modules()}
    seen = 0
    for n, _p in m.named_parameters():
        owner = owners[n.rsplit(".", 1)[0]]
        if n.endswith(("q_norm.weight", "k_norm.weight")):
            assert not hf_decays(n, owner), n
            seen += 1
        elif n.endswith("q_proj.weight"):
            assert hf_decays(n, owner), n
    assert seen == 2 * meta["llm"]["num_hidden_layers"]


def test_qwen3_4b_preset():
    d = resolve_llm_config("Qwen/Qwen3-4B-Instruct-2507")
    cfg = LLMConfig.from_dict(d)
    assert cfg.model_type == "qwen3" and cfg.qk_norm and not cfg.attention_bias
    assert (cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers) == (2560, 9728, 36)
    assert (cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim, cfg.vocab_size) == (32, 8, 128, 151936)
    assert cfg.rms_norm_eps == 1e-6 and cfg.tie_word_embeddings and cfg.max_position_embeddings == 262144
    assert cfg.rope_parameters == {"rope_type": "default", "rope_theta": 5000000.0}


def test_unsupported_qwen3_variants_raise(golden_dir):
    meta, _, _ = load_qwen3_golden("tiny_clip_qwen3", golden_dir)
    with pytest.raises(NotImplementedError):
        LLMConfig.from_dict(dict(meta["llm"], model_type="qwen3_moe"))
    with pytest.raises(NotImplementedError):
        LLMConfig.from_dict(dict(meta["llm"], use_sliding_window=True, layer_types=["sliding_attention", "full_attention"]))


def test_qwen_recipe_builds_model_collator_trainer(tmp_path):
    """The keys of the reference's Qwen alignment recipe; the LLM is a tiny local qwen3 directory standing in for the hub name and
    the BiomedCLIP modality is swapped for meditron_clip (out of scope)."""
    from tests.test_training_config_cpu import ATTACH, alignment_recipe, make_tokenizer, tiny_dirs
    from multimeditron_amd.train import from_training_config
    from multimeditron_amd.train.trainer import TrainingMode
    llm, clips = tiny_dirs(tmp_path)
    cfg = json.load(open(os.path.join(llm, "config.json")))
    cfg.update(model_type="qwen3", rms_norm_eps=1e-6, tie_word_embeddings=True, layer_types=["full_attention"] * cfg["num_hidden_layers"],
               rope_parameters={"rope_type": "default", "rope_theta": 5000000.0})
    json.dump(cfg, open(os.path.join(llm, "config.json"), "w"))
    recipe = alignment_recipe(llm, clips[0])
    recipe.update(tokenizer_type="qwen3", token_size=64)
    recipe["modalities"] = [{"model_type": "meditron_clip", "clip_name": clips[0], "hidden_size": 64}]
    recipe["training_args"]["save_strategy"] = "epoch"
    tok = make_tokenizer()
    setup = from_training_config(recipe, tok, train_dataset=[{"text": "a cat ."}] * 64, device="cpu", dtype="float32")
    model, coll, tr = setup.model, setup.collator, setup.trainer
    llm_cfg = model.model.config
    assert llm_cfg.model_type == "qwen3" and llm_cfg.qk_norm and llm_cfg.tie_word_embeddings
    a = model.model.model.layers[0].self_attn
    assert a.q_norm is not None and a.k_norm is not None and a.q_norm.eps == 1e-6
    assert model.model.lm_head.weight is model.model.model.embed_tokens.weight
    assert coll.chat_template.name == "qwen3" and coll.attachment_token == ATTACH
    assert tr.training_mode == TrainingMode.ALIGNMENT
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    assert trainable and all(".projector." in n for n in trainable)
    assert (tr.lr, tr.wd, tr.max_grad_norm, tr.accum, tr.min_lr, tr.lr_scheduler_type) == (1e-4, 0.01, 1.0, 8, 3e-5, "cosine_with_min_lr")
