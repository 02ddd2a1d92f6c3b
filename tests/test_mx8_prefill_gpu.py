"""The opt-in MXFP8 prefill (forward / generate with prefill_weights="mxfp8") through the model layers.

Wiring, bitwise.  A test-side chain calls the public wrappers in the documented order (DecoderLayer.infer, step=False: rmsnorm_fwd ->
quant_mxfp8 -> gemm_mx8 -> RoPE or q/k norm + RoPE -> cache append -> attn_fwd -> quant -> gemm (+ residual) -> rmsnorm_fwd -> quant
-> gemm -> swiglu_fwd / xielu_fwd -> quant -> gemm (+ residual), then the final norm and the bf16 lm_head); every kernel is
deterministic, so forward(prefill_weights="mxfp8", use_cache=True) must give that chain's logits and cache rows bit for bit, on a
bf16 and on an MXFP8 KV cache.  Tiny 2-layer decoders with head_dim 128 and the smallest widths the GEMM takes (256 and 384: a
packed layout with padding slots, three and more K-stages); B S = 74 rows is no multiple of anything in the tile.

Accuracy, measured.  tests/mx8_ref.py restates the layer in fp64 with the format (tests/w8_check.py) applied to the four GEMM
inputs and the weights; what is left between it and the GPU logits is the GPU path's own rounding (bf16 tensors between kernels)
-- and what that rounding does to the quantiser: an e4m3 element has 3 mantissa bits, so a GEMM input that lands on the other side
of a rounding boundary moves by 2^-4 of its value, and these random-weight decoders (sigma 0.05 at H = 256) amplify it.
rel-L2 of the logits MEASURED on the MI355X: llama 0.0757, qwen2 0.0535, qwen3 0.0886, apertus 0.0716 (the bf16 prefill's logits
are 0.113 / 0.084 / 0.132 / 0.099 away from the same reference: the format's error); REL_L2 = 2x the measured value rounded up to
one significant digit (tests/test_model_gpu.py's rule for format error): 0.2 for all four.

generate on the reference-generated d128 fixture (hidden 128, intermediate 256): reproducible greedy ids; composes with
decode_weights, kv_cache and the seeded device sampler; equals a manual loop (the MX prefill through forward, then the ordinary
decode steps); prefill_weights=None gives the bits of a model that never made the copies.  Refusals and the snapshot rule."""
import pytest
import torch

from multimeditron_amd import kernels as K
from multimeditron_amd._lib import get_option
from oracle import ref_cpu as R
from tests import mx8_ref
from tests.model_utils import build_from_golden

pytestmark = pytest.mark.gpu

MX8 = 23
REL_L2 = {"llama": 0.2, "qwen2": 0.2, "qwen3": 0.2, "apertus": 0.2}
B_, S_ = 2, 37

KINDS = {  # model_type, attention_bias, qk_norm, hidden_act
    "llama": ("llama", False, False, "silu"),
    "qwen2": ("qwen2", True, False, "silu"),
    "qwen3": ("qwen3", False, True, "silu"),
    "apertus": ("apertus", False, True, "xielu"),
}


def _decoder(kind, H=256, I=384, Hq=2, Hkv=1, seed=0):
    from multimeditron_amd.model.llm import CausalLM, LLMConfig
    from multimeditron_amd.nn import FlatParams
    mt, bias, qkn, act = KINDS[kind]
    cfg = LLMConfig(model_type=mt, hidden_size=H, intermediate_size=I, num_hidden_layers=2, num_attention_heads=Hq,
                    num_key_value_heads=Hkv, head_dim=128, vocab_size=1003, attention_bias=bias, qk_norm=qkn, hidden_act=act,
                    pad_token_id=3 if mt == "apertus" else None)
    torch.manual_seed(seed)
    m = CausalLM(cfg, dtype=torch.bfloat16, device="cuda")
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "alpha_" in k:
                continue                                              # xIELU's raw scalars keep their initial values
            p.copy_((torch.randn(p.shape, device="cuda") * (0.3 if p.dim() == 1 else 0.05) + (1.0 if "norm" in k else 0.0)).to(p.dtype))
    FlatParams([(k, p, "llm") for k, p in m.named_parameters()], "cuda", torch.bfloat16)
    return m.eval()


def _ids(m, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(4, m.config.vocab_size, (B_, S_), device="cuda", generator=g)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


@torch.no_grad()
def _chain(m, ids, kv):
    """the documented launch order, from the public wrappers -> (logits2d [B S, V], caches)"""
    cfg = m.config
    B, S = ids.shape
    H, D, T = cfg.hidden_size, cfg.head_dim, B * S
    x = m.model.embed_tokens(ids).reshape(T, H)
    cos, sin = m._tables(torch.arange(S, device="cuda").unsqueeze(0).expand(B, S))
    caches = m.new_cache(B, S + 3, kv_cache=kv)
    kinds = []

    def lin(pk_n, t, **kw):
        out = K.gemm_mx8(K.quant_mxfp8(t), T, pk_n[0], pk_n[1], t.shape[1], **kw)
        kinds.append(get_option("gemm_last_kernel"))
        return out

    for layer, lw, c in zip(m.model.layers, m._decode_w8["layers"], caches):
        a, ml = layer.self_attn, layer.mlp
        Hq, Hkv = a.Hq, a.Hkv
        n1, n2 = layer.norms()
        h, _ = K.rmsnorm_fwd(x, n1.weight, n1.eps)
        qkv = lin(lw["qkv"], h, bias=a._bqkv.tensor() if a._bqkv is not None else None)
        if a.q_norm is not None:
            K.qk_norm_rope_fwd(qkv, T, Hq, Hkv, D, a.q_norm.weight, a.k_norm.weight, a.q_norm.eps, cos, sin, out=qkv, want_rstd=False)
        else:
            K.rope_apply_(qkv, T, Hq + Hkv, D, (Hq + 2 * Hkv) * D, cos, sin)
        q = qkv[:, : Hq * D].view(B, S, Hq, D)
        kn = qkv[:, Hq * D:(Hq + Hkv) * D].view(B, S, Hkv, D)
        vn = qkv[:, (Hq + Hkv) * D:].view(B, S, Hkv, D)
        if kv is None:
            c.k[:, :S].copy_(kn)
            c.v[:, :S].copy_(vn)
        else:
            K.kv8_append(kn, vn, c.buf, c.Smax, 0)
        c.len = S
        o = K.attn_fwd(q, kn, vn, None, True, D ** -0.5)[0].view(T, Hq * D)
        x = lin(lw["o"], o, residual=x)
        h, _ = K.rmsnorm_fwd(x, n2.weight, n2.eps)
        u = lin(lw["gu"], h)
        act = K.xielu_fwd(u, ml.act_fn.alpha_p.data, ml.act_fn.alpha_n.data, *ml.act_fn.consts()) if layer.xielu else K.swiglu_fwd(u, ml.I)
        x = lin(lw["down"], act, residual=x)
    assert kinds == [MX8] * (4 * len(m.model.layers))
    x, _ = K.rmsnorm_fwd(x, m.model.norm.weight, m.model.norm.eps)
    return K.linear_fwd(x, m.lm_head.weight, ldc_pad=True), caches


@pytest.mark.parametrize("kv", [None, "mxfp8"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_forward_is_the_documented_chain_bit_for_bit(kind, kv):
    m = _decoder(kind)
    ids = _ids(m)
    with torch.no_grad():
        base = m(input_ids=ids, use_cache=True, max_new_tokens=3)
        assert m._decode_w8 is None                                   # the default call makes no copies
        out = m(input_ids=ids, use_cache=True, max_new_tokens=3, prefill_weights="mxfp8", kv_cache=kv)
    assert m._decode_w8 is not None                                   # built on first use
    want, caches = _chain(m, ids, kv)
    got = out.logits.reshape(B_ * S_, -1)
    assert bool(torch.isfinite(got.float()).all())
    assert _same_bits(got, want), float((got.float() - want.float()).abs().max())
    assert not _same_bits(got, base.logits.reshape(B_ * S_, -1))      # ... and they are not the bf16 prefill's
    for c, w in zip(out.past_key_values, caches):
        assert c.len == w.len == S_
        if kv is None:
            assert _same_bits(c.k[:, :S_], w.k[:, :S_]) and _same_bits(c.v[:, :S_], w.v[:, :S_])
        else:
            assert torch.equal(c.buf, w.buf)
    with torch.no_grad():                                             # without a cache: the same logits; logits_to_keep: its rows
        nc = m(input_ids=ids, prefill_weights="mxfp8")
        last = m(input_ids=ids, prefill_weights="mxfp8", logits_to_keep=1)
        assert _same_bits(nc.logits, out.logits) and nc.past_key_values is None
        assert _same_bits(last.logits[:, 0], out.logits[:, -1])
        again = m(input_ids=ids, prefill_weights=None)                # the bf16 path after the copies exist: the parent's bits
    assert _same_bits(again.logits, base.logits)


@pytest.mark.parametrize("kind", list(KINDS))
def test_logits_against_the_fp64_restatement(kind):
    m = _decoder(kind, seed=2)
    ids = _ids(m, seed=5)
    with torch.no_grad():
        got = m(input_ids=ids, prefill_weights="mxfp8").logits.double()
        bf = m(input_ids=ids).logits.double()
    ref = mx8_ref.forward(m, ids)
    rel = float((got - ref).norm() / ref.norm())
    fmt = float((bf - ref).norm() / ref.norm())
    print(f"mx8 prefill {kind}: rel-L2 to the fp64 restatement {rel:.4g} (the bf16 prefill's logits are {fmt:.4g} away from it)")
    assert rel <= REL_L2[kind], (kind, rel)


# ---- generate ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(golden_dir):
    return R.load_golden("tiny_clip_llama_d128", golden_dir)


@pytest.fixture(scope="module")
def model_bf16(gold, tmp_path_factory):
    meta, w, v = gold
    return build_from_golden(meta, w, tmp_path_factory.mktemp("mx8m16"), "bfloat16")


@torch.no_grad()
def _manual_loop(m, batch, n_new, temperature=0.1):
    """generate's loop restated: the MX prefill through forward, then the ordinary decode steps"""
    dev = m.device
    input_ids = batch["input_ids"].to(dev)
    B, V, eos = input_ids.shape[0], m._llm_cfg.vocab_size, m.config.eos_token_idx
    nxt = m.embed_modalities_with_text(input_ids, batch["processed_multimodal_inputs"])
    attention_mask = batch["attention_mask"].to(dev)
    position_ids = batch["position_ids"].to(dev)
    L = attention_mask.shape[1]
    cache = m.model.new_cache(B, L + n_new)
    full = torch.ones((B, L + n_new), dtype=attention_mask.dtype, device=dev)
    full[:, :L] = attention_mask
    out_ids = torch.full((B, n_new), eos, dtype=torch.int64, device=dev)
    finished = torch.zeros(B, dtype=torch.uint8, device=dev)
    next_ids = torch.empty(B, dtype=torch.int64, device=dev)
    for i in range(n_new):
        kw = {"prefill_weights": "mxfp8"} if i == 0 else {}
        if i > 0:
            position_ids = torch.full((B, 1), L + i - 1, dtype=torch.long, device=dev)
            attention_mask = full[:, : L + i]
        o = m.model(inputs_embeds=nxt, attention_mask=attention_mask, position_ids=position_ids, past_key_values=cache, use_cache=True,
                    logits_to_keep=1, **kw)
        tok = K.argmax_softmax(o.logits[:, -1, :], V, temperature)
        K.decode_select(tok, finished, eos, out_ids, i, next_ids)
        nxt = m.model.get_input_embeddings()(next_ids.view(B, 1))
    return out_ids.cpu()


def test_generate_with_the_mxfp8_prefill(gold, model_bf16):
    meta, w, v = gold
    m = model_bf16
    batch = R.golden_batch(v, "left")
    B = batch["input_ids"].shape[0]
    m.model.drop_decode_weights()
    base = m.generate(batch, max_new_tokens=6, do_sample=False)
    assert m.model._decode_w8 is None

    ids = m.generate(batch, max_new_tokens=6, do_sample=False, prefill_weights="mxfp8")
    assert ids.dtype == torch.int64 and ids.device.type == "cpu" and ids.shape[0] == B and 1 <= ids.shape[1] <= 6
    snap = m.model._decode_w8
    assert snap is not None
    assert torch.equal(m.generate(batch, max_new_tokens=6, do_sample=False, prefill_weights="mxfp8"), ids)      # run to run
    assert m.model._decode_w8 is snap                                 # reused, not rebuilt
    manual = _manual_loop(m, batch, 6)
    assert torch.equal(ids, manual[:, : ids.shape[1]])                # the first token and every one after it
    # prefill_weights=None: the bits of the run that never made the copies
    assert torch.equal(m.generate(batch, max_new_tokens=6, do_sample=False), base)

    # composes with the decode copies, the MXFP8 cache and the seeded device sampler
    for kw in (dict(decode_weights="mxfp8"), dict(kv_cache="mxfp8"), dict(decode_weights="mxfp8", kv_cache="mxfp8"),
               dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9, seed=7),
               dict(do_sample=True, temperature=0.8, top_k=20, seed=7, decode_weights="mxfp8", kv_cache="mxfp8")):
        kw.setdefault("do_sample", False)
        a = m.generate(batch, max_new_tokens=6, prefill_weights="mxfp8", **kw)
        b = m.generate(batch, max_new_tokens=6, prefill_weights="mxfp8", **kw)
        assert torch.equal(a, b), kw
        assert a.shape[0] == B and 1 <= a.shape[1] <= 6
        if not kw["do_sample"]:
            assert torch.equal(a[:, 0], ids[:, 0]), kw                # the prefill, hence the first token, is shared
    m.model.drop_decode_weights()
    assert torch.equal(m.generate(batch, max_new_tokens=6, do_sample=False), base)


def test_refusals_come_before_the_prefill(gold, model_bf16, tmp_path):
    meta, w, v = gold
    batch = R.golden_batch(v, "left")
    m32 = build_from_golden(meta, w, tmp_path, "float32")
    with pytest.raises(ValueError, match="bfloat16"):
        m32.generate(batch, max_new_tokens=2, do_sample=False, prefill_weights="mxfp8")
    assert m32.model._decode_w8 is None
    with pytest.raises(ValueError, match="int4"):
        model_bf16.generate(batch, max_new_tokens=2, do_sample=False, prefill_weights="int4")
    m = _decoder("llama")
    ids = _ids(m)
    with pytest.raises(ValueError, match="int4"):
        m(input_ids=ids, prefill_weights="int4")
    with torch.enable_grad(), pytest.raises(ValueError, match="autograd"):
        m(input_ids=ids, prefill_weights="mxfp8")
    assert m._decode_w8 is None and "autograd" in m.prefill_weights_ok(B_, S_) and m.prefill_weights_ok(B_, S_, check_grad=False) is None
    odd = _decoder("llama", I=448)                                    # 448 = 3.5 x 128: a K width mm_gemm_mx8 refuses
    with torch.no_grad(), pytest.raises(ValueError, match="448"):
        odd(input_ids=ids, prefill_weights="mxfp8")
    assert odd._decode_w8 is None
    with torch.no_grad():
        assert bool(torch.isfinite(odd(input_ids=ids).logits.float()).all())      # ... while its bf16 prefill runs


def test_snapshot_rule():
    m = _decoder("llama")
    ids = _ids(m)
    with torch.no_grad():
        first = m(input_ids=ids, prefill_weights="mxfp8").logits.clone()
        snap = m._decode_w8
        m(input_ids=ids, prefill_weights="mxfp8")
        assert m._decode_w8 is snap
        m.train()
        assert m._decode_w8 is None
        m.eval()
        wdown = m.model.layers[0].mlp.down_proj.weight
        wdown.mul_(-1.5)
        changed = m(input_ids=ids, prefill_weights="mxfp8").logits.clone()      # rebuilt from the weights as they are now
        assert m._decode_w8 is not None and m._decode_w8 is not snap
        assert not _same_bits(changed, first)
        m.load_state_dict(m.state_dict())
        assert m._decode_w8 is None
        assert _same_bits(m(input_ids=ids, prefill_weights="mxfp8").logits, changed)
