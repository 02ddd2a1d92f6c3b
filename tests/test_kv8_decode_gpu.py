"""The opt-in MXFP8 KV cache through the model layers, held to exact results.

The chain: a decoder keeps its cache in MXFP8 (new_cache(kv_cache="mxfp8")); the SAME decoder runs the shipped bf16 decode step over a
bf16 cache whose rows are replaced, right after every append, by tests/w8_check.roundtrip_ref of themselves.  With one slice per
launch (attn_decode_wgs = 1) the kernels promise the same bits (tests/test_kv8_contract_gpu.py), so the logits must be bit-identical
step after step -- on the fused chain, on the separate launches (MM_DECODE_FUSED=0) and on the q/k-norm path, with bf16 and with
MXFP8 decode weights.  The prefill attends over the unquantised prompt: its logits are the plain bf16 path's.  No tolerance: the
quantisation's own error is a property of the format, not of this code.

generate(..., kv_cache="mxfp8") on the reference-generated d128 fixture: the default path is untouched, shape / determinism / eos
bookkeeping, the size of the buffers, and the refusal of every model that cannot use the cache."""
import json
import os

import pytest
import torch

from multimeditron_amd import kernels as K
from multimeditron_amd.model.llm import CausalLM, LayerKVCache, LayerKVCacheMX8, LLMConfig
from oracle import ref_cpu as R
from tests import w8_check as W8
from tests.kernel_check import options
from tests.model_utils import build_from_golden

pytestmark = pytest.mark.gpu


def _decoder(cfg, seed=0, dtype=torch.bfloat16):
    from multimeditron_amd.nn import FlatParams
    torch.manual_seed(seed)
    m = CausalLM(cfg, dtype=dtype, device="cuda")
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_((torch.randn(p.shape, device="cuda") * (0.3 if p.dim() == 1 else 0.05) + (1.0 if "norm" in k else 0.0)).to(p.dtype))
    FlatParams([(k, p, "llm") for k, p in m.named_parameters()], "cuda", dtype)
    return m.eval()


class RoundtripCache(LayerKVCache):
    """The bf16 cache holding what an MXFP8 cache stands for: every appended row becomes roundtrip_ref of itself before a decode
    step attends over it; the prompt's rows after the prefill has attended over them unquantised."""

    def _roundtrip(self, lo, hi):
        for t in (self.k, self.v):
            rows = t[:, lo:hi].cpu()
            t[:, lo:hi] = W8.roundtrip_ref(rows.reshape(-1, rows.shape[-1])).view(rows.shape).cuda()

    def decode_attend(self, q, key_mask, scale):
        self._roundtrip(self.len, self.len + 1)
        return super().decode_attend(q, key_mask, scale)

    def attend(self, qkv, cos, sin, key_mask, B, S, a):
        out = super().attend(qkv, cos, sin, key_mask, B, S, a)
        if S > 1:
            self._roundtrip(0, self.len)
        return out


def _run(m, cache, ids, S, n_new, **kw):
    """prefill of ids[:, :S] into `cache`, then n_new single-token steps -> [prefill logits, step logits ...]"""
    B = ids.shape[0]
    out = []
    with torch.no_grad():
        o = m(input_ids=ids[:, :S], past_key_values=cache, use_cache=True)
        out.append(o.logits[:, -1].clone())
        for i in range(n_new):
            pos = torch.full((B, 1), S + i, device="cuda", dtype=torch.long)
            o = m(input_ids=ids[:, S + i:S + i + 1], past_key_values=cache, use_cache=True, position_ids=pos, **kw)
            out.append(o.logits[:, -1].clone())
    torch.cuda.synchronize()
    return out


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


# (model_type, Hq, Hkv, qkv bias, H, fused launches)
CHAINS = [("llama", 4, 1, False, 256, True), ("qwen2", 4, 2, True, 1024, True), ("qwen3", 4, 2, False, 256, True),
          ("llama", 4, 2, False, 1024, False), ("qwen2", 4, 1, True, 256, False)]


@pytest.mark.parametrize("mt,Hq,Hkv,bias,H,fused", CHAINS, ids=[f"{c[0]}-{c[1]}x{c[2]}-H{c[4]}-{'fused' if c[5] else 'separate'}" for c in CHAINS])
def test_decode_chain_has_the_bits_of_the_bf16_cache_holding_the_dequantised_rows(mt, Hq, Hkv, bias, H, fused, monkeypatch):
    if not fused:
        monkeypatch.setenv("MM_DECODE_FUSED", "0")
    D = 128
    cfg = LLMConfig(model_type=mt, hidden_size=H, intermediate_size=2 * H + 64, num_hidden_layers=2, num_attention_heads=Hq,
                    num_key_value_heads=Hkv, head_dim=D, vocab_size=1003, attention_bias=bias, qk_norm=mt == "qwen3")
    m = _decoder(cfg)
    assert m.kv_cache_ok(3) is None
    B, S, n_new = 3, 150, 20
    Smax = S + n_new
    torch.manual_seed(1)
    ids = torch.randint(0, cfg.vocab_size, (B, Smax), device="cuda")
    x = torch.empty(B, H, dtype=torch.bfloat16, device="cuda")

    def mx8():
        cache = m.new_cache(B, Smax, kv_cache="mxfp8")
        assert all(type(c) is LayerKVCacheMX8 and c.buf.dtype == torch.uint8 and c.buf.numel() == K.kv8_bytes(B, Smax, Hkv, D) for c in cache)
        return cache

    def held():
        return [RoundtripCache(B, Smax, Hkv, D, torch.bfloat16, "cuda") for _ in range(cfg.num_hidden_layers)]

    with torch.no_grad():
        c0 = mx8()[0]
        assert all(layer.can_decode_step(x, B, 1, c0) for layer in m.model.layers)
        assert all(layer.can_decode_step_fused(x, B, 1, c0) == (fused and mt != "qwen3") for layer in m.model.layers)

    with options(attn_decode_wgs=1):                            # one slice at every length: the slices coincide at every step
        plain = _run(m, m.new_cache(B, Smax), ids, S, n_new)
        got, want = _run(m, mx8(), ids, S, n_new), _run(m, held(), ids, S, n_new)
        assert _same_bits(got[0], plain[0]), "the prefill is not the bf16 path's"
        for i, (p, q) in enumerate(zip(got, want)):
            assert bool(torch.isfinite(q.float()).all())
            assert _same_bits(p, q), (i, float((p.float() - q.float()).abs().max()))
        assert not any(_same_bits(p, q) for p, q in zip(got[1:], plain[1:]))      # ... and they are not the unquantised cache's logits

        m.quantize_decode_weights()
        got8, want8 = (_run(m, c, ids, S, n_new, decode_weights="mxfp8") for c in (mx8(), held()))
        assert _same_bits(got8[0], plain[0])
        for i, (p, q) in enumerate(zip(got8, want8)):
            assert _same_bits(p, q), (i, float((p.float() - q.float()).abs().max()))
        assert not any(_same_bits(p, q) for p, q in zip(got8[1:], got[1:]))

    # forward allocates the cache itself
    with torch.no_grad():
        o = m(input_ids=ids[:, :S], use_cache=True, max_new_tokens=3, kv_cache="mxfp8")
    assert all(type(c) is LayerKVCacheMX8 and c.len == S and c.Smax == S + 3 for c in o.past_key_values)
    assert _same_bits(o.logits[:, -1], plain[0])
    # S > 1 on a cache that holds positions
    with pytest.raises(ValueError, match="MXFP8 KV cache"), torch.no_grad():
        m(input_ids=ids[:, :2], past_key_values=o.past_key_values, use_cache=True)


# ---- generate ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(golden_dir):
    return R.load_golden("tiny_clip_llama_d128", golden_dir)


@pytest.fixture(scope="module")
def model_bf16(gold, tmp_path_factory):
    meta, w, v = gold
    return build_from_golden(meta, w, tmp_path_factory.mktemp("kv8m16"), "bfloat16")


def _one_step_logits(llm, ids, **kw):
    with torch.no_grad():
        cache = llm(input_ids=ids[:, :-1], use_cache=True, max_new_tokens=2, **kw).past_key_values
        pos = torch.full((ids.shape[0], 1), ids.shape[1] - 1, device="cuda", dtype=torch.long)
        return llm(input_ids=ids[:, -1:], past_key_values=cache, use_cache=True, position_ids=pos).logits[:, -1].clone()


def test_generate_with_an_mxfp8_kv_cache(gold, model_bf16, monkeypatch):
    meta, w, v = gold
    m = model_bf16
    batch = R.golden_batch(v, "left")
    B = batch["input_ids"].shape[0]
    eos = m.config.eos_token_idx
    m.model.drop_decode_weights()
    tid = torch.randint(0, meta["llm"]["vocab_size"], (2, 9), generator=torch.Generator().manual_seed(3)).cuda()

    made = []
    new_cache = m.model.new_cache
    monkeypatch.setattr(m.model, "new_cache", lambda *a, **kw: made.append(new_cache(*a, **kw)) or made[-1])

    base = m.generate(batch, max_new_tokens=8, do_sample=False)
    base_logits = _one_step_logits(m.model, tid)
    base_sampled = m.generate(batch, max_new_tokens=8, temperature=0.8, top_k=20, seed=7)
    assert all(type(c) is LayerKVCache for cache in made for c in cache)
    del made[:]

    ids = m.generate(batch, max_new_tokens=8, do_sample=False, kv_cache="mxfp8")
    assert ids.dtype == torch.int64 and ids.device.type == "cpu" and ids.dim() == 2 and ids.shape[0] == B and 1 <= ids.shape[1] <= 8
    assert torch.equal(ids[:, 0], base[:, 0])                    # the prefill is not quantised
    c = m.model.config
    Smax = batch["attention_mask"].shape[1] + 8
    assert len(made) == 1 and len(made[0]) == c.num_hidden_layers
    for lc in made[0]:
        assert type(lc) is LayerKVCacheMX8 and lc.buf.numel() == K.kv8_bytes(B, Smax, c.num_key_value_heads, c.head_dim)
        assert Smax - 8 + ids.shape[1] - 1 <= lc.len <= Smax
    assert torch.equal(m.generate(batch, max_new_tokens=8, do_sample=False, kv_cache="mxfp8"), ids)
    assert m.model._decode_w8 is None

    # the device sampler: a fixed seed reproduces
    s1 = m.generate(batch, max_new_tokens=8, temperature=0.8, top_k=20, seed=7, kv_cache="mxfp8")
    s2 = m.generate(batch, max_new_tokens=8, temperature=0.8, top_k=20, seed=7, kv_cache="mxfp8")
    assert torch.equal(s1, s2) and s1.shape[0] == B and 1 <= s1.shape[1] <= 8
    assert torch.equal(s1[:, 0], base_sampled[:, 0])
    # ... and with the MXFP8 decode weights
    both = m.generate(batch, max_new_tokens=8, do_sample=False, kv_cache="mxfp8", decode_weights="mxfp8")
    assert both.shape[0] == B and 1 <= both.shape[1] <= 8 and torch.equal(both[:, 0], base[:, 0])
    assert torch.equal(m.generate(batch, max_new_tokens=8, do_sample=False, kv_cache="mxfp8", decode_weights="mxfp8"), both)
    m.model.drop_decode_weights()

    # eos bookkeeping: make the token row 0 emits at step 1 the eos; the row then emits eos to the end, the others go on
    assert ids.shape[1] >= 3
    e = int(ids[0, 1])
    m.config.eos_token_idx = e
    try:
        cut = m.generate(batch, max_new_tokens=8, do_sample=False, kv_cache="mxfp8")
        cut16 = m.generate(batch, max_new_tokens=8, do_sample=False)
    finally:
        m.config.eos_token_idx = eos
    for got in (cut, cut16):                                      # the same bookkeeping on both paths
        done = (got == e).to(torch.int8).cummax(dim=1).values.bool()
        assert bool((got[done] == e).all())
        assert bool(done[0, 1:].all())
    first = int((ids[0] == e).nonzero()[0])
    assert torch.equal(cut[0, :first + 1], ids[0, :first + 1])

    # the opt-in leaves no state behind: the default path after = before, ids and logits
    assert torch.equal(m.generate(batch, max_new_tokens=8, do_sample=False), base)
    assert torch.equal(m.generate(batch, max_new_tokens=8, temperature=0.8, top_k=20, seed=7), base_sampled)
    assert _same_bits(_one_step_logits(m.model, tid), base_logits)
    kv8_logits = _one_step_logits(m.model, tid, kv_cache="mxfp8")
    assert bool(torch.isfinite(kv8_logits.float()).all()) and not _same_bits(kv8_logits, base_logits)


def _random_model(meta, tmpdir, llm):
    """the product model of the fixture's geometry with another decoder config, randomly initialised (never run)"""
    from multimeditron_amd.model.modalities import ImageConfig
    from multimeditron_amd.model.model import MultimodalConfig, MultiModalModelForCausalLM
    clip_dir = os.path.join(str(tmpdir), "clip")
    os.makedirs(clip_dir, exist_ok=True)
    size = meta["vision"]["image_size"]
    json.dump({"vision_config": meta["vision"]}, open(os.path.join(clip_dir, "config.json"), "w"))
    json.dump({"size": {"shortest_edge": size}, "crop_size": {"height": size, "width": size}},
              open(os.path.join(clip_dir, "preprocessor_config.json"), "w"))
    cfg = MultimodalConfig(vocab_size=meta["vocab_size"], modalities=[ImageConfig(hidden_size=llm["hidden_size"], clip_name=clip_dir)],
                           llm_path="unused", dtype="bfloat16", eos_token_idx=meta["eos_token_idx"], hidden_size=llm["hidden_size"])
    m = MultiModalModelForCausalLM(cfg, device="cuda", llm_config=llm)
    m.pack_parameters()
    return m


def _refused(m, batch, match, **kw):
    """generate raises ValueError naming the reason before the decoder runs at all"""
    def boom(*a, **k):
        raise AssertionError("the decoder ran")
    m.model.forward = boom
    try:
        with pytest.raises(ValueError, match=match):
            m.generate(batch, max_new_tokens=2, do_sample=False, **kw)
    finally:
        del m.model.forward


def test_generate_refuses_what_cannot_keep_an_mxfp8_cache(gold, model_bf16, golden_dir, tmp_path):
    meta, w, v = gold
    batch = R.golden_batch(v, "left")
    _refused(model_bf16, batch, "fp4", kv_cache="fp4")
    _refused(build_from_golden(meta, w, tmp_path / "f32", "float32"), batch, "bfloat16", kv_cache="mxfp8")
    meta64, w64, v64 = R.load_golden("tiny_clip_llama", golden_dir)
    _refused(build_from_golden(meta64, w64, tmp_path / "d64", "bfloat16"), R.golden_batch(v64, "left"), "head_dim is 64", kv_cache="mxfp8")
    for Hq, Hkv in ((7, 1), (8, 1)):
        llm = dict(meta["llm"], num_attention_heads=Hq, num_key_value_heads=Hkv)
        _refused(_random_model(meta, tmp_path / f"g{Hq}", llm), batch, f"{Hq} query heads on {Hkv}", kv_cache="mxfp8")
    # the decoder's own entry points refuse alike
    cfg = LLMConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=8, num_key_value_heads=1, head_dim=128,
                    vocab_size=64)
    llm = CausalLM(cfg, dtype=torch.bfloat16, device="cuda")
    assert "8 query heads" in llm.kv_cache_ok(2)
    with pytest.raises(ValueError, match="8 query heads"):
        llm.new_cache(2, 16, kv_cache="mxfp8")
    with pytest.raises(ValueError, match="fp4"):
        llm.new_cache(2, 16, kv_cache="fp4")
    assert all(type(c) is LayerKVCache for c in llm.new_cache(2, 16))
