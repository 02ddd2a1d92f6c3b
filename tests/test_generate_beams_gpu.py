"""generate(num_beams=n): beam search over one shared copy of the prompt's keys and values, held to exact results.

The chain: a decoder prefills B prompts ONCE into a LayerKVCacheBeam (new_cache(beams=n, prompt_len=Sp)) and then steps B n rows whose
suffix keys are read through an ancestor table; the SAME decoder steps a plain LayerKVCache of B n rows that the test reorders with
index_select before every step (HF's reorder_cache).  Both are fed the same forced tokens AND forced parents.  With one slice per
launch (attn_decode_wgs = 1) the kernels promise the same bits (tests/test_beam_attn_contract_gpu.py,
tests/test_attn_shared_contract_gpu.py), so the logits must be bit-identical step after step -- on the fused chain, on the separate
launches (MM_DECODE_FUSED=0), on the q/k-norm path, with bf16 and with MXFP8 decode weights.

generate(..., num_beams=n) on the reference-generated d128 fixture equals a slow loop of the test (plain reordered cache, the same
mm_beam_step); sync_every does not matter, steps past "done" change nothing; shapes, order, eos fill, scores; the cache holds the prompt
once; every refusal; num_beams = 1 is today's path."""
import pytest
import torch

from multimeditron_amd import kernels as K
from multimeditron_amd.model.llm import CausalLM, LayerKVCache, LayerKVCacheBeam, LLMConfig
from oracle import ref_cpu as R
from tests.kernel_check import options
from tests.model_utils import build_from_golden
from tests.test_kv8_decode_gpu import _decoder, _random_model, _same_bits

pytestmark = pytest.mark.gpu


# (model_type, Hq, Hkv, qkv bias, fused launches)
CHAINS = [("llama", 4, 1, False, True), ("qwen2", 4, 2, True, True), ("qwen3", 4, 2, False, True), ("llama", 4, 1, False, False),
          ("qwen2", 2, 2, True, False)]


@pytest.mark.parametrize("mt,Hq,Hkv,bias,fused", CHAINS, ids=[f"{c[0]}-{c[1]}x{c[2]}-{'fused' if c[4] else 'separate'}" for c in CHAINS])
def test_beam_chain_has_the_bits_of_the_reordered_cache(mt, Hq, Hkv, bias, fused, monkeypatch):
    if not fused:
        monkeypatch.setenv("MM_DECODE_FUSED", "0")
    D, H, S, n_new, B, n = 128, 256, 70, 7, 2, 3
    cfg = LLMConfig(model_type=mt, hidden_size=H, intermediate_size=2 * H + 64, num_hidden_layers=2, num_attention_heads=Hq,
                    num_key_value_heads=Hkv, head_dim=D, vocab_size=1003, attention_bias=bias, qk_norm=mt == "qwen3")
    m = _decoder(cfg)
    assert m.beams_ok(B, n) is None
    R_, Smax = B * n, S + n_new
    torch.manual_seed(1)
    ids = torch.randint(0, cfg.vocab_size, (B, S), device="cuda")
    tok = torch.randint(0, cfg.vocab_size, (R_, n_new), device="cuda")          # forced ids, different in every row
    base = torch.arange(R_, device="cuda") // n * n
    par = base[None, :] + torch.randint(0, n, (n_new, R_), device="cuda")        # forced parents (physical rows), inside each prompt
    par[2] = base + n - 1                                                         # once: every beam continues one row
    pmask = torch.ones(B, S, dtype=torch.long, device="cuda")
    pmask[0, :7] = 0                                                              # a left-padded prompt

    def pos(i):
        return torch.full((R_, 1), S + i, device="cuda", dtype=torch.long)

    def beam(**kw):
        cache = m.new_cache(B, Smax, beams=n, prompt_len=S)
        assert all(type(c) is LayerKVCacheBeam and c.tables is cache[0].tables and c.ks.shape == (R_, n_new, Hkv, D) for c in cache)
        out = []
        with torch.no_grad():
            first = m(input_ids=ids, attention_mask=pmask, past_key_values=cache, use_cache=True).logits[:, -1].clone()
            table = torch.zeros(n_new, R_, dtype=torch.int32, device="cuda")
            for i in range(n_new):
                if i > 0:                                                         # what mm_beam_step writes for the coming step
                    table[:i] = table[:i].index_select(1, par[i])
                table[i] = torch.arange(R_, dtype=torch.int32, device="cuda")
                cache[0].tables.current = table.clone()
                out.append(m(input_ids=tok[:, i:i + 1], past_key_values=cache, use_cache=True, position_ids=pos(i), attention_mask=pmask,
                             **kw).logits[:, -1].clone())
        torch.cuda.synchronize()
        return cache, first, out

    def plain(src, **kw):
        cache = m.new_cache(R_, Smax)
        for c, s in zip(cache, src):
            c.k[:, :S], c.v[:, :S], c.len = s.k[:, :S].repeat_interleave(n, 0), s.v[:, :S].repeat_interleave(n, 0), S
        out = []
        with torch.no_grad():
            for i in range(n_new):
                if i > 0:                                                         # reorder_cache: every layer, every token
                    for c in cache:
                        c.k.copy_(c.k.index_select(0, par[i]))
                        c.v.copy_(c.v.index_select(0, par[i]))
                mask = torch.cat([pmask.repeat_interleave(n, 0), torch.ones(R_, i + 1, dtype=torch.long, device="cuda")], 1)
                out.append(m(input_ids=tok[:, i:i + 1], past_key_values=cache, use_cache=True, position_ids=pos(i), attention_mask=mask,
                             **kw).logits[:, -1].clone())
        torch.cuda.synchronize()
        return out

    with options(attn_decode_wgs=1):                            # one slice in both launches at every length
        with torch.no_grad():
            want_first = m(input_ids=ids, attention_mask=pmask, past_key_values=m.new_cache(B, Smax), use_cache=True).logits[:, -1].clone()
        bc, first, got = beam()
        assert _same_bits(first, want_first), "the prefill is not the plain cache's"
        want = plain(bc)
        assert all(c.slen == n_new for c in bc)
        for i, (p, q) in enumerate(zip(got, want)):
            assert bool(torch.isfinite(q.float()).all())
            assert _same_bits(p, q), (i, float((p.float() - q.float()).abs().max()))
        # the table matters: the same tokens without reordering give other logits
        _, _, straight = beam_straight(m, B, n, S, Smax, ids, tok, pmask, pos, n_new)
        assert not _same_bits(straight[-1], got[-1])

        m.quantize_decode_weights()
        bc8, _, got8 = beam(decode_weights="mxfp8")
        want8 = plain(bc8, decode_weights="mxfp8")
        for i, (p, q) in enumerate(zip(got8, want8)):
            assert _same_bits(p, q), (i, float((p.float() - q.float()).abs().max()))
        assert not any(_same_bits(p, q) for p, q in zip(got8, got))

    with pytest.raises(ValueError, match="ancestor table"), torch.no_grad():
        c = m.new_cache(B, Smax, beams=n, prompt_len=S)
        m(input_ids=ids, attention_mask=pmask, past_key_values=c, use_cache=True)
        m(input_ids=tok[:, :1], past_key_values=c, use_cache=True, attention_mask=pmask)


def beam_straight(m, B, n, S, Smax, ids, tok, pmask, pos, n_new):
    """the beam cache under the identity table (every row continues itself)"""
    cache = m.new_cache(B, Smax, beams=n, prompt_len=S)
    out = []
    with torch.no_grad():
        first = m(input_ids=ids, attention_mask=pmask, past_key_values=cache, use_cache=True).logits[:, -1].clone()
        cache[0].tables.current = torch.arange(B * n, dtype=torch.int32, device="cuda")[None, :].expand(n_new, B * n).contiguous()
        for i in range(n_new):
            out.append(m(input_ids=tok[:, i:i + 1], past_key_values=cache, use_cache=True, position_ids=pos(i), attention_mask=pmask).logits[:, -1].clone())
    return cache, first, out


# ---- generate ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(golden_dir):
    return R.load_golden("tiny_clip_llama_d128", golden_dir)


@pytest.fixture(scope="module")
def model_bf16(gold, tmp_path_factory):
    meta, w, v = gold
    return build_from_golden(meta, w, tmp_path_factory.mktemp("beams16"), "bfloat16")


def slow_beams(m, batch, T, n, nrs, length_penalty, early_stopping, eos):
    """generate(num_beams=n) restated with a plain cache of B n rows reordered by index_select, the same mm_beam_step, no early exit"""
    dev = m.device
    llm = m.model
    with torch.no_grad():
        input_ids = batch["input_ids"].to(dev)
        B = input_ids.shape[0]
        R_ = B * n
        V = llm.config.vocab_size
        x = m.embed_modalities_with_text(input_ids, batch["processed_multimodal_inputs"])
        pmask = batch["attention_mask"].to(dev)
        S = pmask.shape[1]
        small = llm.new_cache(B, S + T)
        logits = llm(inputs_embeds=x, attention_mask=pmask, position_ids=batch["position_ids"].to(dev), past_key_values=small,
                     use_cache=True, logits_to_keep=1).logits[:, -1, :]
        cache = llm.new_cache(R_, S + T)
        for c, s in zip(cache, small):
            c.k[:, :S], c.v[:, :S], c.len = s.k[:, :S].repeat_interleave(n, 0), s.v[:, :S].repeat_interleave(n, 0), S
        st = K.BeamState(B, n, T, V, dev)
        base = torch.arange(R_, device=dev) // n * n
        emb = llm.get_input_embeddings()
        for i in range(T):
            nxt = K.beam_step(logits, st, i, eos, length_penalty, early_stopping)
            if i + 1 == T:
                break
            order = base + st.parent.long()
            if i > 0:                                             # the rows written so far follow their beams
                for c in cache:
                    c.k.copy_(c.k.index_select(0, order))
                    c.v.copy_(c.v.index_select(0, order))
            mask = torch.cat([pmask.repeat_interleave(n, 0), torch.ones(R_, i + 1, dtype=pmask.dtype, device=dev)], 1)
            pos = torch.full((R_, 1), S + i, dtype=torch.long, device=dev)      # padded prompt length + (i + 1) - 1
            logits = llm(inputs_embeds=emb(nxt.view(R_, 1)), attention_mask=mask, position_ids=pos, past_key_values=cache, use_cache=True,
                         logits_to_keep=1).logits[:, -1, :]
        ids, scores, lens = K.beam_finish(st, nrs, eos)
        n_out = int(lens.max())
        return ids[:, :n_out].cpu(), scores.cpu()


def test_generate_beams_is_the_slow_loop(gold, model_bf16, monkeypatch):
    meta, w, v = gold
    m = model_bf16
    batch = R.golden_batch(v, "left")
    B = batch["input_ids"].shape[0]
    eos0 = m.config.eos_token_idx
    m.model.drop_decode_weights()
    T = 8
    base = m.generate(batch, max_new_tokens=T, do_sample=False)
    base_sampled = m.generate(batch, max_new_tokens=T, temperature=0.8, top_k=20, seed=7)

    made, asked = [], []
    new_cache = m.model.new_cache

    def spy(*a, **kw):
        asked.append((a, kw))
        made.append(new_cache(*a, **kw))
        return made[-1]

    monkeypatch.setattr(m.model, "new_cache", spy)
    # num_beams = 1 is today's path, bit for bit
    assert torch.equal(m.generate(batch, max_new_tokens=T, do_sample=False, num_beams=1), base)
    assert torch.equal(m.generate(batch, max_new_tokens=T, temperature=0.8, top_k=20, seed=7, num_beams=1), base_sampled)
    assert all(type(c) is LayerKVCache for cache in made for c in cache) and all("beams" not in kw for _, kw in asked)
    del made[:], asked[:]

    with options(attn_decode_wgs=1):
        n = 4
        ids, scores = m.generate(batch, max_new_tokens=T, do_sample=False, num_beams=n, num_return_sequences=n, return_beam_scores=True)
        assert asked[0][1].get("beams") == n and len(made) == 1
        # the memory claim: the prompt once per prompt, the generated tokens once per beam row
        c = m.model.config
        Sp = batch["attention_mask"].shape[1]
        for lc in made[0]:
            assert type(lc) is LayerKVCacheBeam and lc.len == Sp
            nbytes = sum(t.numel() * t.element_size() for t in (lc.k, lc.v, lc.ks, lc.vs))
            assert nbytes == 2 * c.num_key_value_heads * c.head_dim * 2 * (B * Sp + B * n * T)
        monkeypatch.undo()
        assert ids.dtype == torch.int64 and ids.device.type == "cpu" and ids.shape[0] == B * n and 1 <= ids.shape[1] <= T
        assert scores.dtype == torch.float32 and scores.shape == (B * n,) and bool(torch.isfinite(scores).all())
        for b in range(B):
            s = scores[b * n:(b + 1) * n]
            assert bool((s[:-1] >= s[1:]).all()), s                               # descending per prompt
        want_ids, want_scores = slow_beams(m, batch, T, n, n, 1.0, False, eos0)
        assert torch.equal(ids, want_ids) and torch.equal(scores.view(torch.int32), want_scores.view(torch.int32))
        one = m.generate(batch, max_new_tokens=T, do_sample=False, num_beams=n)
        assert one.shape[0] == B and torch.equal(one, ids[::n, :one.shape[1]]) and bool((ids[::n, one.shape[1]:] == eos0).all())

        # eos made the best continuation of every row from the fourth call of the decoder on (a test-only bonus on its logit, seen by
        # generate and by the slow loop alike): every beam ends there, the call is done before max_new_tokens, the host notices at its
        # next look (sync_every), and the steps issued past "done" -- which still offer eos everywhere -- change nothing
        calls = []
        fwd = m.model.forward

        def pushing(*a, **kw):
            calls.append(1)
            out = fwd(*a, **kw)
            if len(calls) >= 4:
                out.logits[:, -1, eos0] = 30.0
            return out

        for es, lp in ((True, 1.0), (False, 0.0), ("never", 1.0)):
            runs = {}
            m.model.forward = pushing
            try:
                for se in (1, 3, 16):
                    del calls[:]
                    runs[se] = m.generate(batch, max_new_tokens=T, do_sample=False, num_beams=2, num_return_sequences=2, sync_every=se,
                                          early_stopping=es, length_penalty=lp, return_beam_scores=True) + (len(calls),)
                del calls[:]
                want_ids, want_scores = slow_beams(m, batch, T, 2, 2, lp, es, eos0)
            finally:
                del m.model.forward
            for se in (3, 16):
                assert torch.equal(runs[se][0], runs[1][0]) and torch.equal(runs[se][1], runs[1][1]), (es, lp, se)
            assert torch.equal(runs[1][0], want_ids) and torch.equal(runs[1][1], want_scores), (es, lp)
            assert runs[16][2] == T
            got = runs[1][0]
            ended = (got == eos0).to(torch.int8).cummax(dim=1).values.bool()
            assert bool((got[ended] == eos0).all())                               # eos included, eos behind the end
            if es != "never":
                assert runs[1][2] == 4 and runs[3][2] == 6, (es, runs[1][2], runs[3][2])      # done at the fourth step
                assert got.shape[1] == 4 and bool((got[:, 3] == eos0).all())

    # with the MXFP8 decode and prefill weights
    both = m.generate(batch, max_new_tokens=T, do_sample=False, num_beams=4, decode_weights="mxfp8")
    assert both.shape[0] == B and 1 <= both.shape[1] <= T
    pre = m.generate(batch, max_new_tokens=T, do_sample=False, num_beams=4, prefill_weights="mxfp8")
    assert pre.shape[0] == B and 1 <= pre.shape[1] <= T
    m.model.drop_decode_weights()
    # the opt-in leaves no state behind
    assert torch.equal(m.generate(batch, max_new_tokens=T, do_sample=False), base)
    assert torch.equal(m.generate(batch, max_new_tokens=T, temperature=0.8, top_k=20, seed=7), base_sampled)
    empty, es_ = m.generate(batch, max_new_tokens=0, do_sample=False, num_beams=2, num_return_sequences=2, return_beam_scores=True)
    assert empty.shape == (2 * B, 0) and es_.shape == (2 * B,)


def test_generate_sixteen_beams_over_a_long_table(gold, model_bf16):
    """16 beams x 24 tokens: a table of more than 256 entries per prompt, evolved by mm_beam_step alone (the second trip of its copy
    loops), goes through LayerKVCacheBeam into mm_attn_decode_beam; ids and score bits are the slow loop's (a plain reordered cache),
    whatever sync_every"""
    meta, w, v = gold
    m = model_bf16
    batch = R.golden_batch(v, "left")
    B = batch["input_ids"].shape[0]
    eos0 = m.config.eos_token_idx
    m.model.drop_decode_weights()
    n, T = 16, 24
    assert (T - 1) * n > 256 and m.model.beams_ok(B, n) is None
    calls = []
    fwd = m.model.forward

    def counting(*a, **kw):
        calls.append(1)
        return fwd(*a, **kw)

    with options(attn_decode_wgs=1):
        runs, steps = {}, {}
        m.model.forward = counting
        try:
            for se in (1, 16):
                del calls[:]
                runs[se] = m.generate(batch, max_new_tokens=T, do_sample=False, num_beams=n, num_return_sequences=n, early_stopping="never",
                                      sync_every=se, return_beam_scores=True)
                steps[se] = len(calls)
        finally:
            del m.model.forward
        want_ids, want_scores = slow_beams(m, batch, T, n, n, 1.0, "never", eos0)
    ids, scores = runs[1]
    assert ids.shape[0] == B * n and torch.equal(ids, want_ids) and torch.equal(scores.view(torch.int32), want_scores.view(torch.int32))
    assert torch.equal(runs[16][0], ids) and torch.equal(runs[16][1].view(torch.int32), scores.view(torch.int32))
    print(f"decoder calls: {steps}")
    assert (steps[1] - 1) * n > 256, steps                                        # the run went past 256 table entries per prompt


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


def test_generate_refuses_what_beam_search_cannot_do(gold, model_bf16, golden_dir, tmp_path):
    meta, w, v = gold
    batch = R.golden_batch(v, "left")
    B = batch["input_ids"].shape[0]
    g = dict(do_sample=False)
    for bad in (0, -1, 17, 2.0, True, "4"):
        _refused(model_bf16, batch, r"num_beams must be an int in \[1, 16\]", num_beams=bad, **g)
    _refused(model_bf16, batch, "do_sample=False", num_beams=2)                   # generate's default samples
    _refused(model_bf16, batch, "do_sample=False", num_beams=2, do_sample=True)
    for k, val in (("top_k", 5), ("top_p", 0.9), ("min_p", 0.1), ("seed", 3), ("generator", torch.Generator())):
        _refused(model_bf16, batch, f"with {k}", num_beams=2, **g, **{k: val})
    _refused(model_bf16, batch, "out of scope", num_beams=2, kv_cache="mxfp8", **g)
    _refused(model_bf16, batch, "num_return_sequences=3 > num_beams=2", num_beams=2, num_return_sequences=3, **g)
    for bad in (float("inf"), float("nan"), "1", None, True):
        _refused(model_bf16, batch, "length_penalty must be a finite number", num_beams=2, length_penalty=bad, **g)
    for bad in (1, 0, "always", None):
        _refused(model_bf16, batch, "early_stopping must be", num_beams=2, early_stopping=bad, **g)
    _refused(model_bf16, batch, "return_beam_scores needs num_beams > 1", return_beam_scores=True, **g)
    # today's refusal stands with num_beams = 1
    _refused(model_bf16, batch, "do_sample=True", do_sample=False, num_return_sequences=2, num_beams=1)
    # a model samples_ok refuses; a vocabulary below 2 n
    _refused(build_from_golden(meta, w, tmp_path / "f32", "float32"), batch, "bfloat16", num_beams=2, **g)
    meta64, w64, v64 = R.load_golden("tiny_clip_llama", golden_dir)
    _refused(build_from_golden(meta64, w64, tmp_path / "d64", "bfloat16"), R.golden_batch(v64, "left"), "head_dim is 64", num_beams=2, **g)
    llm = dict(meta["llm"], num_attention_heads=8, num_key_value_heads=1)
    _refused(_random_model(meta, tmp_path / "g8", llm), batch, "8 query heads on 1", num_beams=2, **g)
    n16 = 16 // B + 1
    if n16 <= 16:
        _refused(model_bf16, batch, f"batch of {B * n16} sequences", decode_weights="mxfp8", num_beams=n16, **g)
    # the decoder's own entry points refuse alike
    cfg = LLMConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1, head_dim=128,
                    vocab_size=20)
    llm = CausalLM(cfg, dtype=torch.bfloat16, device="cuda")
    assert llm.beams_ok(2, 10) is None and "vocab_size is 20" in llm.beams_ok(2, 11)
    with pytest.raises(ValueError, match="vocab_size is 20"):
        llm.new_cache(2, 16, beams=11, prompt_len=8)
    with pytest.raises(ValueError, match="bf16 only"):
        llm.new_cache(2, 16, kv_cache="mxfp8", beams=3, prompt_len=8)
    with pytest.raises(ValueError, match="prompt_len"):
        llm.new_cache(2, 16, beams=3)
    with pytest.raises(ValueError, match="beams must be"):
        llm.new_cache(2, 16, beams=0)
    assert all(type(c) is LayerKVCache for c in llm.new_cache(2, 16, beams=1))
    assert all(type(c) is LayerKVCacheBeam for c in llm.new_cache(2, 16, beams=3, prompt_len=8))
