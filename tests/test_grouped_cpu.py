"""Grouped launches (the expert as a batch dimension) without a GPU: the six `*_batched` entry points exist in header and library,
they reject bad arguments before any launch, and the `grouped_towers` switch of the MoE modalities round-trips through the config
and arrives from a training recipe."""
import ctypes

import pytest

from multimeditron_amd import _lib

BATCHED = ("mm_gemm_batched", "mm_gemm_act_fwd_batched", "mm_colsum_batched", "mm_layernorm_fwd_batched", "mm_layernorm_bwd_batched",
           "mm_reduce_partials2_batched")
ERR_ARG, ERR_ALIGN = -1, -2


def _arr(n, value=64):
    """a host array of n fake, 64-byte-aligned device pointers: never dereferenced, the calls below fail before any launch"""
    return (ctypes.c_void_p * n)(*[value * (i + 1) for i in range(n)])


def test_header_and_library_agree():
    protos = _lib.parse_header()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in BATCHED:
        assert name in protos, f"include/mm_hip.h does not declare {name}"
        assert hasattr(L, name), f"libmmhip.so does not export {name}"
    src = open(_lib.HEADER).read()
    assert "MM_GROUP_MAX = 16" in src and _lib.GROUP_MAX == 16


@pytest.mark.parametrize("groups", [0, 17])
def test_group_count_is_checked(groups):
    L = _lib.lib()
    a = _arr(17)
    assert L.mm_gemm_batched(0, 0, groups, 32, 32, 32, a, 32, a, 32, a, 32, None, None, 0, 0, None) == ERR_ARG
    assert L.mm_gemm_act_fwd_batched(0, groups, 32, 32, 32, a, 32, a, 32, a, a, 32, a, 32, None, 0, 1 | 4, None) == ERR_ARG
    assert L.mm_colsum_batched(0, a, groups, 32, 32, 32, a, 0, None) == ERR_ARG
    assert L.mm_layernorm_fwd_batched(0, 64, a, a, groups, 4, 128, 1e-5, 64, 64, 64, None) == ERR_ARG
    assert L.mm_layernorm_bwd_batched(0, 64, 64, a, groups, 64, 64, 4, 128, 64, 64, 64, None, None) == ERR_ARG
    assert L.mm_reduce_partials2_batched(0, 64, 64, groups, 1, 128, a, a, 0, 0, None) == ERR_ARG


def test_null_pointer_arrays_are_rejected():
    L = _lib.lib()
    a = _arr(3)
    hole = (ctypes.c_void_p * 3)(64, None, 192)
    for A, B, C in ((None, a, a), (a, None, a), (a, a, None), (hole, a, a), (a, a, hole)):
        assert L.mm_gemm_batched(0, 0, 3, 32, 32, 32, A, 32, B, 32, C, 32, None, None, 0, 0, None) == ERR_ARG
    assert L.mm_gemm_batched(0, 0, 3, 32, 32, 32, a, 32, a, 32, a, 32, None, None, 0, 1, None) == ERR_ARG          # MM_EPI_BIAS without bias[]
    assert L.mm_gemm_batched(0, 0, 3, 32, 32, 32, a, 32, a, 32, a, 32, None, None, 32, 8, None) == ERR_ARG         # MM_EPI_RESIDUAL without residual[]
    assert L.mm_gemm_act_fwd_batched(0, 3, 32, 32, 32, a, 32, a, 32, a, None, 32, a, 32, None, 0, 1 | 4, None) == ERR_ARG      # no PRE[]
    assert L.mm_colsum_batched(0, None, 3, 32, 32, 32, a, 0, None) == ERR_ARG
    assert L.mm_colsum_batched(0, a, 3, 32, 32, 32, hole, 0, None) == ERR_ARG
    assert L.mm_layernorm_fwd_batched(0, 64, None, a, 3, 4, 128, 1e-5, 64, 64, 64, None) == ERR_ARG
    assert L.mm_layernorm_fwd_batched(0, 64, a, None, 3, 4, 128, 1e-5, 64, 64, 64, None) == ERR_ARG
    assert L.mm_layernorm_bwd_batched(0, 64, 64, hole, 3, 64, 64, 4, 128, 64, 64, 64, None, None) == ERR_ARG
    assert L.mm_reduce_partials2_batched(0, 64, 64, 3, 1, 128, a, None, 0, 0, None) == ERR_ARG


def test_alignment_is_checked_before_any_launch():
    L = _lib.lib()
    a = _arr(3)
    assert L.mm_gemm_batched(0, 0, 3, 32, 32, 32, a, 3, a, 32, a, 32, None, None, 0, 0, None) == ERR_ALIGN          # lda = 3
    odd = (ctypes.c_void_p * 3)(64, 130, 192)                                                                       # problem 1's A at 2 mod 16
    assert L.mm_gemm_batched(0, 0, 3, 32, 32, 32, odd, 32, a, 32, a, 32, None, None, 0, 0, None) == ERR_ALIGN
    assert L.mm_gemm_act_fwd_batched(0, 3, 32, 32, 32, a, 3, a, 32, a, a, 32, a, 32, None, 0, 1 | 4, None) == ERR_ALIGN
    assert L.mm_colsum_batched(0, a, 3, 32, 32, 3, a, 0, None) == ERR_ALIGN
    assert L.mm_layernorm_fwd_batched(0, 64, a, a, 3, 4, 12, 1e-5, 64, 64, 64, None) == ERR_ALIGN                   # H % 8
    assert L.mm_reduce_partials2_batched(0, 64, 64, 3, 1, 6, a, a, 0, 0, None) == ERR_ALIGN                         # H % 4


@pytest.mark.parametrize("pep", [False, True])
def test_grouped_towers_config_field(pep):
    from multimeditron_amd.model.modalities import MOEImageConfig, MOEImageConfigPEP
    cls = MOEImageConfigPEP if pep else MOEImageConfig
    assert "grouped_towers" not in cls().to_dict() and cls().grouped_towers is False
    assert "grouped_towers" not in cls(grouped_towers=False).to_dict()
    d = cls(grouped_towers=True).to_dict()
    assert d["grouped_towers"] is True and "train_gate" not in d
    assert cls.from_dict(d).grouped_towers is True and cls.from_dict(cls().to_dict()).grouped_towers is False
    assert list(cls().to_dict()) == [k for k in cls(grouped_towers=True).to_dict() if k != "grouped_towers"]       # nothing else moves


def test_environment_overrides_the_config_field(monkeypatch):
    from multimeditron_amd.model.expert_towers import _grouped_on
    monkeypatch.delenv("MM_MOE_GROUPED", raising=False)
    assert _grouped_on(True) and not _grouped_on(False)
    monkeypatch.setenv("MM_MOE_GROUPED", "1")
    assert _grouped_on(True) and _grouped_on(False)
    monkeypatch.setenv("MM_MOE_GROUPED", "0")
    assert not _grouped_on(True) and not _grouped_on(False)


@pytest.mark.parametrize("model_type", ["moe_meditron_clip_shared", "moe_meditron_clip_pep"])
def test_recipe_key_reaches_the_config(tmp_path, model_type):
    from multimeditron_amd.train import from_training_config
    from tests.test_training_config_cpu import ATTACH, make_tokenizer, tiny_dirs
    llm, clips = tiny_dirs(tmp_path, n_clip=3)
    for flag in (True, None):
        mod = {"model_type": model_type, "image_processor": clips[0], "hidden_size": 64, "expert_clip_names": clips, "generalist_idx": -1,
               "gating_path": "stub", "fusion_method": "weighted_average", "top_k_experts": 3, "cross_attn_heads": 2}
        if flag is not None:
            mod["grouped_towers"] = flag
        recipe = {"base_llm": llm, "base_model": None, "attachment_token": ATTACH, "tokenizer_type": "llama", "token_size": 64,
                  "loaders": [{"loader_type": "raw-image", "modality_type": "image"}], "modalities": [mod], "training_mode": "FULL",
                  "training_args": {"learning_rate": 1.0e-5, "per_device_train_batch_size": 2, "max_steps": 5}}
        setup = from_training_config(recipe, make_tokenizer(), device="cpu", dtype="float32")
        cfg = setup.model.modalities_by_type["image"].config
        assert cfg.grouped_towers is bool(flag)
        assert ("grouped_towers" in cfg.to_dict()) == bool(flag)
        setup.trainer.close()
