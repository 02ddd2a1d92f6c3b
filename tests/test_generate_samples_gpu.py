"""generate(num_return_sequences=n): n samples per prompt over one shared copy of the prompt's keys and values, held to exact results.

The chain: a decoder prefills B prompts ONCE into a LayerKVCacheShared (new_cache(samples=n, prompt_len=Sp)) and then steps B n rows;
the SAME decoder steps a plain LayerKVCache of B n rows whose prompt rows are the shared prefill's rows repeated n times by the test.
Both are fed the same forced token ids, different in every sample row.  With one slice per launch (attn_decode_wgs = 1) the kernels
promise the same bits (tests/test_attn_shared_contract_gpu.py), so the logits must be bit-identical step after step -- on the fused
chain, on the separate launches (MM_DECODE_FUSED=0), on the q/k-norm path, on the generic path (18 rows), with bf16 and with MXFP8
decode weights.  The prefill's logits are those of a plain cache of B rows.

generate(..., num_return_sequences=n) on the reference-generated d128 fixture: n = 1 is today's path, shape / order / determinism /
eos bookkeeping, the size of the cache (the memory claim), and the refusal of every call that cannot use it."""
import pytest
import torch

from multimeditron_amd.model.llm import CausalLM, LayerKVCache, LayerKVCacheShared, LLMConfig
from oracle import ref_cpu as R
from tests.kernel_check import options
from tests.model_utils import build_from_golden
from tests.test_kv8_decode_gpu import _decoder, _random_model, _same_bits

pytestmark = pytest.mark.gpu


def _steps(m, cache, tok, S, mask_of_step, **kw):
    """one forced token per row and step over `cache` (which holds S prompt positions) -> [step logits ...]"""
    rows, out = tok.shape[0], []
    with torch.no_grad():
        for i in range(tok.shape[1]):
            pos = torch.full((rows, 1), S + i, device="cuda", dtype=torch.long)
            o = m(input_ids=tok[:, i:i + 1], past_key_values=cache, use_cache=True, position_ids=pos, attention_mask=mask_of_step(i), **kw)
            out.append(o.logits[:, -1].clone())
    torch.cuda.synchronize()
    return out


# (model_type, Hq, Hkv, qkv bias, fused launches, B, n)
CHAINS = [("llama", 4, 1, False, True, 2, 3), ("qwen2", 4, 2, True, True, 2, 3), ("qwen3", 4, 2, False, True, 2, 3),
          ("llama", 4, 1, False, False, 2, 3), ("qwen2", 4, 2, True, False, 2, 3), ("qwen3", 4, 2, False, False, 2, 3),
          ("llama", 4, 1, False, True, 3, 6), ("qwen2", 4, 2, True, True, 3, 6), ("qwen3", 4, 2, False, True, 3, 6)]


@pytest.mark.parametrize("mt,Hq,Hkv,bias,fused,B,n", CHAINS,
                         ids=[f"{c[0]}-{c[1]}x{c[2]}-{'fused' if c[4] else 'separate'}-B{c[5]}-n{c[6]}" for c in CHAINS])
def test_shared_chain_has_the_bits_of_the_replicated_cache(mt, Hq, Hkv, bias, fused, B, n, monkeypatch):
    if not fused:
        monkeypatch.setenv("MM_DECODE_FUSED", "0")
    D, H, S, n_new = 128, 256, 150, 12
    cfg = LLMConfig(model_type=mt, hidden_size=H, intermediate_size=2 * H + 64, num_hidden_layers=2, num_attention_heads=Hq,
                    num_key_value_heads=Hkv, head_dim=D, vocab_size=1003, attention_bias=bias, qk_norm=mt == "qwen3")
    m = _decoder(cfg)
    assert m.samples_ok(B, n) is None
    R_, Smax = B * n, S + n_new
    torch.manual_seed(1)
    ids = torch.randint(0, cfg.vocab_size, (B, S), device="cuda")
    tok = torch.randint(0, cfg.vocab_size, (R_, n_new), device="cuda")         # forced ids, different in every sample row
    pmask = torch.ones(B, S, dtype=torch.long, device="cuda")
    pmask[0, :7] = 0                                                          # a left-padded prompt
    x = torch.empty(R_, H, dtype=torch.bfloat16, device="cuda")

    def shared():
        cache = m.new_cache(B, Smax, samples=n, prompt_len=S)
        for c in cache:
            assert type(c) is LayerKVCacheShared and c.k.shape == (B, S, Hkv, D) and c.ks.shape == (R_, n_new, Hkv, D)
        with torch.no_grad():
            o = m(input_ids=ids, attention_mask=pmask, past_key_values=cache, use_cache=True)
        assert all(c.len == S and c.slen == 0 for c in cache)
        return cache, o.logits[:, -1].clone()

    def replicated(src):
        cache = m.new_cache(R_, Smax)
        for c, s in zip(cache, src):
            c.k[:, :S], c.v[:, :S], c.len = s.k[:, :S].repeat_interleave(n, 0), s.v[:, :S].repeat_interleave(n, 0), S
        return cache

    def rmask(i):
        return torch.cat([pmask.repeat_interleave(n, 0), torch.ones(R_, i + 1, dtype=torch.long, device="cuda")], 1)

    with torch.no_grad():
        c0 = m.new_cache(B, Smax, samples=n, prompt_len=S)[0]
        assert all(layer.can_decode_step(x, R_, 1, c0) == (R_ <= 16) for layer in m.model.layers)
        assert all(layer.can_decode_step_fused(x, R_, 1, c0) == (R_ <= 16 and fused and mt != "qwen3") for layer in m.model.layers)

    with options(attn_decode_wgs=1):                            # one slice in both launches at every length
        with torch.no_grad():
            plain = m(input_ids=ids, attention_mask=pmask, past_key_values=m.new_cache(B, Smax), use_cache=True).logits[:, -1].clone()
        sc, first = shared()
        assert _same_bits(first, plain), "the prefill is not the plain cache's"
        want = _steps(m, replicated(sc), tok, S, rmask)
        got = _steps(m, sc, tok, S, lambda i: pmask)
        assert all(c.slen == n_new for c in sc)
        for i, (p, q) in enumerate(zip(got, want)):
            assert bool(torch.isfinite(q.float()).all())
            assert _same_bits(p, q), (i, float((p.float() - q.float()).abs().max()))
        assert not _same_bits(got[-1][0], got[-1][1])           # sample rows of one prompt have gone different ways

        if R_ <= 16:
            m.quantize_decode_weights()
            sc8, _ = shared()
            want8 = _steps(m, replicated(sc8), tok, S, rmask, decode_weights="mxfp8")
            got8 = _steps(m, sc8, tok, S, lambda i: pmask, decode_weights="mxfp8")
            for i, (p, q) in enumerate(zip(got8, want8)):
                assert _same_bits(p, q), (i, float((p.float() - q.float()).abs().max()))
            assert not any(_same_bits(p, q) for p, q in zip(got8, got))

    # S > 1 on a shared cache that holds positions; a step beyond the room for generated tokens
    with pytest.raises(ValueError, match="shared-prefix KV cache"), torch.no_grad():
        m(input_ids=ids[:, :2], past_key_values=sc, use_cache=True)
    with pytest.raises(ValueError, match="is full"), torch.no_grad():
        m(input_ids=tok[:, :1], past_key_values=sc, use_cache=True, attention_mask=pmask)


# ---- generate ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(golden_dir):
    return R.load_golden("tiny_clip_llama_d128", golden_dir)


@pytest.fixture(scope="module")
def model_bf16(gold, tmp_path_factory):
    meta, w, v = gold
    return build_from_golden(meta, w, tmp_path_factory.mktemp("samples16"), "bfloat16")


def test_generate_returns_n_samples_per_prompt(gold, model_bf16, monkeypatch):
    meta, w, v = gold
    m = model_bf16
    batch = R.golden_batch(v, "left")
    B = batch["input_ids"].shape[0]
    eos = m.config.eos_token_idx
    m.model.drop_decode_weights()
    n, new = 3, 8

    made, asked = [], []
    new_cache = m.model.new_cache

    def spy(*a, **kw):
        asked.append((a, kw))
        made.append(new_cache(*a, **kw))
        return made[-1]

    monkeypatch.setattr(m.model, "new_cache", spy)

    base = m.generate(batch, max_new_tokens=new, do_sample=False)
    base_sampled = m.generate(batch, max_new_tokens=new, temperature=0.8, top_k=20, seed=7)
    assert all(type(c) is LayerKVCache for cache in made for c in cache) and all("samples" not in kw for _, kw in asked)
    # n = 1 is today's path, greedy and sampled
    assert torch.equal(m.generate(batch, max_new_tokens=new, do_sample=False, num_return_sequences=1), base)
    assert torch.equal(m.generate(batch, max_new_tokens=new, temperature=0.8, top_k=20, seed=7, num_return_sequences=1), base_sampled)
    assert all("samples" not in kw for _, kw in asked)
    del made[:], asked[:]

    ids = m.generate(batch, max_new_tokens=new, temperature=1.0, seed=7, num_return_sequences=n)
    assert ids.dtype == torch.int64 and ids.device.type == "cpu" and ids.dim() == 2 and ids.shape[0] == n * B and 1 <= ids.shape[1] <= new
    assert asked[0][1].get("samples") == n and len(made) == 1
    # the memory claim: the prompt once per prompt, the generated tokens once per sample row
    c = m.model.config
    Sp = batch["attention_mask"].shape[1]
    assert len(made[0]) == c.num_hidden_layers
    for lc in made[0]:
        assert type(lc) is LayerKVCacheShared and lc.len == Sp and ids.shape[1] - 1 <= lc.slen <= new - 1
        nbytes = sum(t.numel() * t.element_size() for t in (lc.k, lc.v, lc.ks, lc.vs))
        assert nbytes == 2 * c.num_key_value_heads * c.head_dim * 2 * (B * Sp + B * n * new)
    assert torch.equal(m.generate(batch, max_new_tokens=new, temperature=1.0, seed=7, num_return_sequences=n), ids)
    assert not torch.equal(m.generate(batch, max_new_tokens=new, temperature=1.0, seed=8, num_return_sequences=n), ids)
    for b in range(B):                                            # the samples of a prompt differ at T = 1
        rows = ids[b * n:(b + 1) * n]
        assert not bool((rows == rows[0]).all()), (b, rows)
    # the torch.multinomial path draws per row too
    torch.manual_seed(5)
    t1 = m.generate(batch, max_new_tokens=new, temperature=1.0, num_return_sequences=n)
    torch.manual_seed(5)
    assert torch.equal(m.generate(batch, max_new_tokens=new, temperature=1.0, num_return_sequences=n), t1) and t1.shape[0] == n * B
    # ... and with the MXFP8 decode and prefill weights
    both = m.generate(batch, max_new_tokens=new, temperature=1.0, seed=7, num_return_sequences=n, decode_weights="mxfp8")
    assert both.shape[0] == n * B and 1 <= both.shape[1] <= new and torch.equal(both[:, 0], ids[:, 0])      # the prefill reads bf16 weights
    pre = m.generate(batch, max_new_tokens=new, temperature=1.0, seed=7, num_return_sequences=n, prefill_weights="mxfp8")
    assert pre.shape[0] == n * B and 1 <= pre.shape[1] <= new
    m.model.drop_decode_weights()

    # eos bookkeeping per row: make the token row 0 emits at step 1 the eos; the row then emits eos to the end, its siblings go on
    assert ids.shape[1] >= 3
    e = int(ids[0, 1])
    m.config.eos_token_idx = e
    try:
        cut = m.generate(batch, max_new_tokens=new, temperature=1.0, seed=7, num_return_sequences=n)
    finally:
        m.config.eos_token_idx = eos
    done = (cut == e).to(torch.int8).cummax(dim=1).values.bool()
    assert bool((cut[done] == e).all()) and bool(done[0, 1:].all())
    assert cut.shape[0] == n * B and cut.shape[1] >= 3
    for r in range(n * B):                                        # the same draws up to a row's first eos
        hit = (ids[r] == e).nonzero()
        upto = min(int(hit[0]) + 1 if len(hit) else ids.shape[1], cut.shape[1])
        assert torch.equal(cut[r, :upto], ids[r, :upto]), r
    assert not bool(done[:, 1].all())                             # a row that ended did not end the others

    # the opt-in leaves no state behind
    assert torch.equal(m.generate(batch, max_new_tokens=new, do_sample=False), base)
    assert torch.equal(m.generate(batch, max_new_tokens=new, temperature=0.8, top_k=20, seed=7), base_sampled)


def _refused(m, batch, match, **kw):
    """generate raises ValueError naming the reason before the decoder runs at all"""
    def boom(*a, **k):
        raise AssertionError("the decoder ran")
    m.model.forward = boom
    try:
        with pytest.raises(ValueError, match=match):
            m.generate(batch, max_new_tokens=2, **kw)
    finally:
        del m.model.forward


def test_generate_refuses_what_cannot_share_a_prefix(gold, model_bf16, golden_dir, tmp_path):
    meta, w, v = gold
    batch = R.golden_batch(v, "left")
    B = batch["input_ids"].shape[0]
    _refused(model_bf16, batch, "do_sample=True", do_sample=False, num_return_sequences=2)
    for bad in (0, -1, 2.0, True):
        _refused(model_bf16, batch, "num_return_sequences must be an int >= 1", num_return_sequences=bad)
    _refused(model_bf16, batch, "out of scope", kv_cache="mxfp8", num_return_sequences=2)
    _refused(build_from_golden(meta, w, tmp_path / "f32", "float32"), batch, "bfloat16", num_return_sequences=2)
    meta64, w64, v64 = R.load_golden("tiny_clip_llama", golden_dir)
    _refused(build_from_golden(meta64, w64, tmp_path / "d64", "bfloat16"), R.golden_batch(v64, "left"), "head_dim is 64", num_return_sequences=2)
    for Hq, Hkv in ((7, 1), (8, 1)):
        llm = dict(meta["llm"], num_attention_heads=Hq, num_key_value_heads=Hkv)
        _refused(_random_model(meta, tmp_path / f"g{Hq}", llm), batch, f"{Hq} query heads on {Hkv}", num_return_sequences=2)
    n16 = 16 // B + 1
    _refused(model_bf16, batch, f"batch of {B * n16} sequences", decode_weights="mxfp8", num_return_sequences=n16)
    # the decoder's own entry points refuse alike
    cfg = LLMConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=8, num_key_value_heads=1, head_dim=128,
                    vocab_size=64)
    llm = CausalLM(cfg, dtype=torch.bfloat16, device="cuda")
    assert "8 query heads" in llm.samples_ok(2, 3)
    with pytest.raises(ValueError, match="8 query heads"):
        llm.new_cache(2, 16, samples=3, prompt_len=8)
    cfg = LLMConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1, head_dim=128,
                    vocab_size=64)
    llm = CausalLM(cfg, dtype=torch.bfloat16, device="cuda")
    assert llm.samples_ok(2, 3) is None
    with pytest.raises(ValueError, match="bf16 only"):
        llm.new_cache(2, 16, kv_cache="mxfp8", samples=3, prompt_len=8)
    with pytest.raises(ValueError, match="prompt_len"):
        llm.new_cache(2, 16, samples=3)
    with pytest.raises(ValueError, match="samples must be"):
        llm.new_cache(2, 16, samples=0)
    assert all(type(c) is LayerKVCache for c in llm.new_cache(2, 16, samples=1))
    assert all(type(c) is LayerKVCacheShared for c in llm.new_cache(2, 16, samples=3, prompt_len=8))
