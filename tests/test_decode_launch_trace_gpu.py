"""Which launches a prefill and two decode steps queue, by name and in order, on every route CausalLM.forward can take.

The bit tests of the inference chains (test_model_gpu, test_w8_decode_gpu, test_kv8_decode_gpu, test_mx8_prefill_gpu,
test_generate_samples_gpu) would still pass if a route quietly fell from the fused decode chain to the separate launches, or from
the append kernel to rope_apply_ + copy_: those give the same bits from more launches.  Here the C-ABI symbol names that pass through
multimeditron_amd.kernels.call are recorded (names only: the arguments are the bit tests' business) and compared with sequences
written out by hand from the chains the docstrings of DecoderLayer.infer / forward, the KV caches' attend / step and
CausalLM.forward document: a per-layer pattern times the number of layers, between the prologue (embedding gather, RoPE table) and
the head (final norm, lm_head).

Tiny decoders (2 layers, hidden 256, intermediate 384, 2 query heads on 1 key/value head of 128, vocab 1003), a prompt of B = 2,
S = 37 (74 rows: below every fused-training-GEMM threshold, so a generic linear is one mm_gemm).  Nothing is timed."""
import pytest
import torch

from multimeditron_amd import kernels as K

pytestmark = pytest.mark.gpu

L_, B_, S_ = 2, 2, 37

KINDS = {  # model_type, attention_bias, qk_norm, hidden_act
    "llama": ("llama", False, False, "silu"),
    "qwen2": ("qwen2", True, False, "silu"),
    "qwen3": ("qwen3", False, True, "silu"),
    "apertus": ("apertus", False, True, "xielu"),
}


def _decoder(kind, dtype=torch.bfloat16, intermediate=384):
    from multimeditron_amd.model.llm import CausalLM, LLMConfig
    from multimeditron_amd.nn import FlatParams
    mt, bias, qkn, act = KINDS[kind]
    cfg = LLMConfig(model_type=mt, hidden_size=256, intermediate_size=intermediate, num_hidden_layers=L_, num_attention_heads=2,
                    num_key_value_heads=1, head_dim=128, vocab_size=1003, attention_bias=bias, qk_norm=qkn, hidden_act=act,
                    pad_token_id=3 if mt == "apertus" else None)
    torch.manual_seed(0)
    m = CausalLM(cfg, dtype=dtype, device="cuda")
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "alpha_" in k:
                continue                                              # xIELU's raw scalars keep their initial values
            p.copy_((torch.randn(p.shape, device="cuda") * (0.3 if p.dim() == 1 else 0.05) + (1.0 if "norm" in k else 0.0)).to(p.dtype))
    FlatParams([(k, p, "llm") for k, p in m.named_parameters()], "cuda", dtype)
    return m.eval()


# ---- the expected sequences, by hand ---------------------------------------------------------------------------------------------
PROLOGUE = ["mm_embed_check_ids", "mm_embed_splice_fwd", "mm_rope_table"]      # the embedding gather (with its id check), cos / sin
NORM, GEMM = "mm_rmsnorm_fwd", "mm_gemm"
MX8 = ["mm_quant_mxfp8", "mm_gemm_mx8"]                                         # one linear of the MXFP8 prefill
W8 = "mm_decode_linear_w8"


def _act(kind):
    return "mm_xielu_fwd" if kind == "apertus" else "mm_swiglu_fwd"


def _qk_norm(kind):
    return kind in ("qwen3", "apertus")


def prefill(kind, lin, kv8=False):
    """forward() with a cache (lin = [GEMM]) or infer on the "prefill" plan (lin = MX8): norm, q|k|v, RoPE (+ q/k norm) in place, the
    cache's store (copy_, or the MXFP8 quantiser), attn_fwd, o_proj, norm, gate|up, activation, down_proj; then the final norm and the bf16
    lm_head."""
    rope = "mm_qk_norm_rope_fwd" if _qk_norm(kind) else "mm_rope_apply"
    layer = [NORM, *lin, rope, *(["mm_kv8_append"] if kv8 else []), "mm_attn_fwd", *lin, NORM, *lin, _act(kind), *lin]
    return PROLOGUE + layer * L_ + [NORM, GEMM]


def step(kind, lin, attend):
    """infer on a separate step: norm, q|k|v, RoPE (+ q/k norm) + cache append in one launch, the cache's decode attention, o_proj, norm,
    gate|up, activation, down_proj; then the final norm and lm_head as the same kind of linear."""
    append = "mm_qk_norm_rope_append" if _qk_norm(kind) else "mm_rope_append"
    layer = [NORM, lin, append, *attend, lin, NORM, lin, _act(kind), lin]
    return PROLOGUE + layer * L_ + [NORM, lin]


def fused_step(sfx, attend):
    """infer on a fused step: norm + q|k|v + RoPE + append, the cache's decode attention, o_proj, norm + gate|up + SwiGLU, down_proj;
    then final norm + lm_head as one launch.  sfx: "" or "_w8"."""
    lin = "mm_decode_linear" + sfx
    layer = ["mm_decode_qkv_rope_append" + sfx, *attend, lin, "mm_decode_gateup_swiglu" + sfx, lin]
    return PROLOGUE + layer * L_ + [lin]


ATTEND = {None: ["mm_attn_decode"], "mxfp8": ["mm_kv8_append", "mm_attn_decode_kv8"], "shared": ["mm_attn_decode_shared"]}


def expected(kind, fused, dw, kv, pw, samples=1):
    pre = prefill(kind, MX8 if pw else [GEMM], kv8=kv is not None)
    attend = ATTEND["shared" if samples > 1 else kv]
    if fused and not _qk_norm(kind):                 # q/k-norm layers never take the fused chain
        one = fused_step("_w8" if dw else "", attend)
    else:
        one = step(kind, W8 if dw else GEMM, attend)
    return [pre, one, one]


# ---- recording -----------------------------------------------------------------------------------------------------------------
def _trace(monkeypatch, m, cache, rows, n_rows_step, **kw):
    """the names of one prefill of `rows` prompts and two steps of n_rows_step rows each, as three lists"""
    g = torch.Generator(device="cuda").manual_seed(1)
    ids = torch.randint(4, m.config.vocab_size, (rows, S_), device="cuda", generator=g)
    nxt = torch.randint(4, m.config.vocab_size, (n_rows_step, 2), device="cuda", generator=g)
    names = []
    call = K.call

    def recording(name, *args):
        names.append(name)
        return call(name, *args)

    monkeypatch.setattr(K, "call", recording)
    out = []
    with torch.no_grad():
        for x in (ids, nxt[:, :1], nxt[:, 1:]):
            del names[:]
            o = m(input_ids=x, past_key_values=cache, use_cache=True, logits_to_keep=1, **kw)
            out.append(list(names))
    torch.cuda.synchronize()
    monkeypatch.setattr(K, "call", call)
    assert bool(torch.isfinite(o.logits.float()).all())
    return out


def _show(got, want):
    return "\n".join(f"call {i}:\n  got  {g}\n  want {w}" for i, (g, w) in enumerate(zip(got, want)) if g != w)


# kind, MM_DECODE_FUSED, decode_weights, kv_cache, prefill_weights
CASES = [("llama", "1", None, None, None), ("llama", "0", None, None, None), ("qwen2", "1", None, None, None),
         ("qwen2", "0", None, None, None), ("qwen3", "1", None, None, None), ("apertus", "1", None, None, None),
         ("llama", "1", "mxfp8", None, None), ("llama", "0", "mxfp8", None, None), ("qwen3", "1", "mxfp8", None, None),
         ("llama", "1", None, "mxfp8", None), ("llama", "0", None, "mxfp8", None), ("apertus", "1", None, "mxfp8", None),
         ("llama", "1", None, None, "mxfp8"), ("apertus", "0", None, None, "mxfp8"),
         ("llama", "1", "mxfp8", "mxfp8", "mxfp8"), ("qwen2", "0", "mxfp8", "mxfp8", "mxfp8"), ("qwen3", "1", "mxfp8", "mxfp8", "mxfp8"),
         ("apertus", "1", "mxfp8", "mxfp8", "mxfp8")]


def _id(c):
    return "-".join([c[0], "fused" if c[1] == "1" else "separate"] + [n for n, v in zip(("dw", "kv", "pw"), c[2:5]) if v])


@pytest.mark.parametrize("kind,fused,dw,kv,pw", CASES, ids=[_id(c) for c in CASES])
def test_prefill_and_two_steps_queue_the_documented_launches(kind, fused, dw, kv, pw, monkeypatch):
    monkeypatch.setenv("MM_DECODE_FUSED", fused)
    m = _decoder(kind)
    if dw or pw:
        m.quantize_decode_weights()                                   # outside the recording: forward would make them on first use
    kw = {k: v for k, v in (("decode_weights", dw), ("prefill_weights", pw)) if v}
    got = _trace(monkeypatch, m, m.new_cache(B_, S_ + 3, kv_cache=kv), B_, B_, **kw)
    want = expected(kind, fused == "1", dw, kv, pw)
    assert got == want, _show(got, want)


@pytest.mark.parametrize("kind,fused,dw", [("llama", "1", None), ("llama", "1", "mxfp8"), ("llama", "0", "mxfp8"), ("qwen3", "1", None)],
                         ids=["llama-fused", "llama-fused-dw", "llama-separate-dw", "qwen3"])
def test_samples_over_a_shared_prompt_cache(kind, fused, dw, monkeypatch):
    """new_cache(samples=3, prompt_len=37): the prefill runs on the 2 prompts, the steps on the 6 sample rows."""
    monkeypatch.setenv("MM_DECODE_FUSED", fused)
    n = 3
    m = _decoder(kind)
    if dw:
        m.quantize_decode_weights()
    kw = {"decode_weights": dw} if dw else {}
    got = _trace(monkeypatch, m, m.new_cache(B_, S_ + 3, samples=n, prompt_len=S_), B_, B_ * n, **kw)
    want = expected(kind, fused == "1", dw, None, None, samples=n)
    assert got == want, _show(got, want)


@pytest.mark.parametrize("fused", ["1", "0"], ids=["llama-fused", "llama-separate"])
def test_beams_read_the_shared_prompt_cache_through_the_ancestor_table(fused, monkeypatch):
    """new_cache(beams=3, prompt_len=37): the steps of test_samples_over_a_shared_prompt_cache with mm_attn_decode_beam as their
    attention (the ancestor table here: every row continues itself)."""
    monkeypatch.setenv("MM_DECODE_FUSED", fused)
    n = 3
    m = _decoder("llama")
    cache = m.new_cache(B_, S_ + 3, beams=n, prompt_len=S_)
    cache[0].tables.current = torch.arange(B_ * n, dtype=torch.int32, device="cuda").repeat(2, 1)
    got = _trace(monkeypatch, m, cache, B_, B_ * n)
    attend = ["mm_attn_decode_beam"]
    one = fused_step("", attend) if fused == "1" else step("llama", GEMM, attend)
    want = [prefill("llama", [GEMM]), one, one]
    assert got == want, _show(got, want)


def verify(kind, fused, lin, down=None):
    """One verify step of a prompt-lookup cache, every position's logits kept.  Separate: norm, q|k|v, RoPE (+ q/k norm) in place,
    the append of the new rows at the rows' own slots, the verify attention, o_proj, norm, gate|up, activation, down_proj; the final
    norm and lm_head.  Fused: norm + q|k|v as one streaming launch (RoPE, append and attention stay: the slots are known on the device
    only), o_proj, norm + gate|up + SwiGLU, down_proj (`down`: the launch that takes it), final norm + lm_head."""
    rope = "mm_qk_norm_rope_fwd" if _qk_norm(kind) else "mm_rope_apply"
    attend = [rope, "mm_kv_append_at", "mm_attn_decode_verify"]
    if fused:
        sfx = "_w8" if lin == W8 else ""
        layer = [lin, *attend, lin, "mm_decode_gateup_swiglu" + sfx, down or lin]
        return PROLOGUE + layer * L_ + [lin]
    layer = [NORM, lin, *attend, lin, NORM, lin, _act(kind), lin]
    return PROLOGUE + layer * L_ + [NORM, lin]


# kind, MM_DECODE_FUSED, decode_weights, intermediate size, sequences, (whether the step is fused, its linear, fused down_proj's launch)
VERIFY = [("llama", "1", None, 384, 2, (True, "mm_decode_linear", None)),
          ("llama", "0", None, 384, 2, (False, GEMM, None)),
          ("qwen3", "1", None, 384, 2, (False, GEMM, None)),                       # q/k-norm layers never take the fused chain
          ("llama", "1", "mxfp8", 384, 2, (True, W8, None)),
          # 4 x 4 = 16 rows of 4608 features exceed the weight-streaming kernel's LDS stage: down_proj is mm_gemm's M <= 16 kernel
          ("llama", "1", None, 4608, 4, (True, "mm_decode_linear", GEMM))]


@pytest.mark.parametrize("kind,fused,dw,inter,B,want", VERIFY, ids=["llama-fused", "llama-separate", "qwen3", "llama-fused-dw", "llama-fused-I4608-16rows"])
def test_a_verify_step_on_a_prompt_lookup_cache(kind, fused, dw, inter, B, want, monkeypatch):
    """new_cache(lookup=3): the prefill is the plain cache's; a verify step brings Q = 4 positions for each of B sequences (as
    the decode loop does, the test sets the rows' base positions: every row stands at the end of its prompt)."""
    monkeypatch.setenv("MM_DECODE_FUSED", fused)
    Q = 4
    m = _decoder(kind, intermediate=inter)
    if dw:
        m.quantize_decode_weights()
    cache = m.new_cache(B, S_ + 2 * Q, lookup=Q - 1)
    g = torch.Generator(device="cuda").manual_seed(1)
    ids = torch.randint(4, m.config.vocab_size, (B, S_ + Q), device="cuda", generator=g)
    names, call = [], K.call

    def recording(name, *args):
        names.append(name)
        return call(name, *args)

    with torch.no_grad():
        m(input_ids=ids[:, :S_], past_key_values=cache, use_cache=True, logits_to_keep=1)
        cache[0].shared.base, cache[0].shared.bound = torch.full((B,), S_, dtype=torch.int32, device="cuda"), S_
        pos = (torch.arange(Q, device="cuda") + S_).unsqueeze(0).expand(B, Q)
        monkeypatch.setattr(K, "call", recording)
        o = m(input_ids=ids[:, S_:], past_key_values=cache, use_cache=True, position_ids=pos, **({"decode_weights": dw} if dw else {}))
        monkeypatch.setattr(K, "call", call)
    torch.cuda.synchronize()
    assert o.logits.shape[:2] == (B, Q) and bool(torch.isfinite(o.logits.float()).all())
    assert names == verify(kind, *want), _show([names], [verify(kind, *want)])


@pytest.mark.parametrize("kind", ["llama", "qwen2"])
def test_a_one_token_prompt_enters_the_empty_lookup_cache_as_a_decode_step(kind, monkeypatch):
    """S = 1 into a prompt-lookup cache that holds nothing (its base positions already set, as generate's loop does): the fused decode
    step of the plain cache, q|k|v bias included, writing slot 0 -- not a verify step."""
    monkeypatch.setenv("MM_DECODE_FUSED", "1")
    m = _decoder(kind)
    cache = m.new_cache(B_, 12, lookup=3)
    cache[0].shared.base, cache[0].shared.bound = torch.ones(B_, dtype=torch.int32, device="cuda"), 1
    ids = torch.randint(4, m.config.vocab_size, (B_, 1), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    names, call = [], K.call

    def recording(name, *args):
        names.append(name)
        return call(name, *args)

    monkeypatch.setattr(K, "call", recording)
    with torch.no_grad():
        o = m(input_ids=ids, past_key_values=cache, use_cache=True, logits_to_keep=1)
    monkeypatch.setattr(K, "call", call)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o.logits.float()).all()) and all(c.len == 1 for c in cache)
    assert names == fused_step("", ATTEND[None]), _show([names], [fused_step("", ATTEND[None])])


def test_seventeen_rows_take_the_generic_route(monkeypatch):
    """One row more than the decode step accepts: every step is forward() over the cache -- RoPE in place, copy_ into the cache,
    the decode attention (one new position), and the norms, linears and SwiGLU as launches of their own."""
    monkeypatch.setenv("MM_DECODE_FUSED", "1")
    m = _decoder("llama")
    got = _trace(monkeypatch, m, m.new_cache(17, S_ + 3), 17, 17)
    layer = [NORM, GEMM, "mm_rope_apply", "mm_attn_decode", GEMM, NORM, GEMM, "mm_swiglu_fwd", GEMM]
    one = PROLOGUE + layer * L_ + [NORM, GEMM]
    # the prefill has 17 x 37 = 629 rows, past the 256 from which the gate|up GEMM carries SwiGLU in its epilogue (kernels.gemm_swiglu_fwd)
    layer = [NORM, GEMM, "mm_rope_apply", "mm_attn_fwd", GEMM, NORM, "mm_gemm_swiglu_fwd", GEMM]
    want = [PROLOGUE + layer * L_ + [NORM, GEMM], one, one]
    assert got == want, _show(got, want)


def test_an_fp32_model_takes_the_generic_route(monkeypatch):
    """fp32 has no decode-step kernels: a step is forward() over the cache, and its one new position is attended by attn_fwd."""
    monkeypatch.setenv("MM_DECODE_FUSED", "1")
    m = _decoder("llama", dtype=torch.float32)
    got = _trace(monkeypatch, m, m.new_cache(B_, S_ + 3), B_, B_)
    want = [prefill("llama", [GEMM])] * 3
    assert got == want, _show(got, want)
