"""generate(guidance_scale=, negative_batch=) on the reference-generated d128 fixture (B = 2, Sc = 200, row 1 left-padded).

generate is the slow loop: the same ids as a loop built here from the pieces generate had before guidance -- two plain LayerKVCache
prefills of B rows (the unconditional one at its own length Su), their rows copied with torch into one plain LayerKVCache of 2 B rows
at the right-aligned slots, plain steps of 2 B rows under the mask and the per-row positions of the feature, K.cfg_combine, then the
existing selection --, for HF's default negative prompt (the last id), an image-less negative batch (Su < Sc, one row shorter than
the other) and a negative batch longer than the prompt; greedy, the device sampler, the processors, MXFP8 decode weights, both
sync_every, an eos that ends one row early.  The semantics, independent of the plumbing: at step 0 the combined scores lie inside
tests/cfg_check.py's bound of the fp64 formula on the logits of two separate plain forward calls.  It does something; off is off;
one decoder call per step; every refusal before anything is encoded."""
import math

import pytest
import torch

from multimeditron_amd import kernels as K
from multimeditron_amd.model import llm as llm_mod
from oracle import ref_cpu as R
from tests import cfg_check as CC
from tests.model_utils import build_from_golden

pytestmark = pytest.mark.gpu

NEW = 8
NO_MM = {"batch_idx": {}, "token_range": {}, "stacked": {}}


@pytest.fixture(scope="module")
def gold(golden_dir):
    return R.load_golden("tiny_clip_llama_d128", golden_dir)


@pytest.fixture(scope="module")
def model(gold, tmp_path_factory):
    meta, w, v = gold
    return build_from_golden(meta, w, tmp_path_factory.mktemp("cfg16"), "bfloat16")


@pytest.fixture(scope="module")
def batch(gold):
    b = R.golden_batch(gold[2], "left")
    assert b["input_ids"].shape == (2, 200) and int((b["attention_mask"][1] == 0).sum()) == 7
    return b


@pytest.fixture(scope="module")
def plain(model, batch):
    model.model.drop_decode_weights()
    return model.generate(batch, max_new_tokens=NEW, do_sample=False)


def _left_padded(rows, pad):
    S = max(len(r) for r in rows)
    ids = torch.full((len(rows), S), pad, dtype=torch.int64)
    mask = torch.zeros((len(rows), S), dtype=torch.int64)
    for r, row in enumerate(rows):
        ids[r, S - len(row):] = torch.as_tensor(row)
        mask[r, S - len(row):] = 1
    return dict(input_ids=ids, attention_mask=mask, position_ids=(mask.cumsum(1) - 1).clamp(min=0), processed_multimodal_inputs=NO_MM)


def _negative(batch, kind, pad):
    """None; "text": the batch with its image spans removed and re-padded on the left (184 and 161 visible ids); "long": the same
    behind 30 more ids (Su = 214 > Sc)"""
    if kind == "last":
        return None
    ids, pmi = batch["input_ids"], batch["processed_multimodal_inputs"]
    keep = batch["attention_mask"].bool().clone()
    keep[pmi["batch_idx"]["image"], pmi["token_range"]["image"]] = False
    rows = [ids[r][keep[r]].tolist() for r in range(ids.shape[0])]
    if kind == "long":
        rows = [[(7 * j + 3 * r) % 120 for j in range(30)] + row for r, row in enumerate(rows)]
    neg = _left_padded(rows, pad)
    assert [int(n) for n in neg["attention_mask"].sum(1)] == ([184, 161] if kind == "text" else [214, 191])
    return neg


# ---- the slow loop, from the pieces generate had before guidance -------------------------------------------------------------------
def _slow(m, batch, neg, scale, select, dw=None, processors=None):
    """-> ids [B, NEW] on the host (untrimmed), the step-0 (cond logits, uncond logits, scores)"""
    llm, dev = m.model, m.device
    emb = llm.get_input_embeddings()
    V, eos = m._llm_cfg.vocab_size, m.config.eos_token_idx
    dwk = {"decode_weights": dw} if dw else {}
    with torch.no_grad():
        ids = batch["input_ids"].to(dev)
        B, Sc = ids.shape
        cmask = batch["attention_mask"].to(dev)
        feeds = [dict(inputs_embeds=m.embed_modalities_with_text(ids, batch["processed_multimodal_inputs"]), attention_mask=cmask,
                      position_ids=batch["position_ids"].to(dev))]
        if neg is None:
            feeds.append(dict(inputs_embeds=emb(ids[:, -1:]), attention_mask=torch.ones((B, 1), dtype=cmask.dtype, device=dev),
                              position_ids=torch.zeros((B, 1), dtype=torch.long, device=dev)))
        else:
            feeds.append(dict(inputs_embeds=m.embed_modalities_with_text(neg["input_ids"].to(dev), neg["processed_multimodal_inputs"]),
                              attention_mask=neg["attention_mask"].to(dev), position_ids=neg["position_ids"].to(dev)))
        Su = feeds[1]["attention_mask"].shape[1]
        Sp = max(Sc, Su)
        halves, logits = [], []
        for f in feeds:                                        # two plain prefills of B rows, each at its own length
            c = llm.new_cache(B, f["attention_mask"].shape[1] + 1)
            assert type(c[0]) is llm_mod.LayerKVCache
            logits.append(llm(past_key_values=c, use_cache=True, logits_to_keep=1, **f, **dwk).logits[:, -1, :])
            halves.append(c)
        big = llm.new_cache(2 * B, Sp + NEW)                   # one plain cache of 2 B rows, both halves right-aligned
        assert type(big[0]) is llm_mod.LayerKVCache
        for layer, (cc, cu) in zip(big, zip(*halves)):
            layer.k[:B, Sp - Sc:Sp], layer.v[:B, Sp - Sc:Sp] = cc.k[:, :Sc], cc.v[:, :Sc]
            layer.k[B:, Sp - Su:Sp], layer.v[B:, Sp - Su:Sp] = cu.k[:, :Su], cu.v[:, :Su]
            layer.len = Sp
        mask = torch.zeros((2 * B, Sp + NEW), dtype=cmask.dtype, device=dev)
        mask[:, Sp:] = 1
        mask[:B, Sp - Sc:Sp], mask[B:, Sp - Su:Sp] = cmask, feeds[1]["attention_mask"]
        pos = torch.tensor([[Sc]] * B + [[Su]] * B, dtype=torch.long, device=dev)
        st = K.GuidanceState(B, V, dev)
        lp = K.LogitsState(B, V, dev, *processors, prompt_ids=ids, prompt_mask=cmask, room=NEW) if processors else None
        out = torch.full((B, NEW), eos, dtype=torch.int64)
        finished = torch.zeros(B, dtype=torch.bool)
        nxt, first = None, None
        x = torch.cat(logits)
        for i in range(NEW):
            if i > 0:
                x = llm(past_key_values=big, use_cache=True, inputs_embeds=emb(nxt.repeat(2).view(2 * B, 1)), attention_mask=mask[:, :Sp + i],
                        position_ids=pos + (i - 1), logits_to_keep=1, **dwk).logits[:, -1, :]
            scores = K.cfg_combine(x, st, scale)
            if i == 0:
                first = (x[:B].clone(), x[B:].clone(), scores.clone())
            if lp is not None:
                scores = K.logits_process(scores, lp, i, nxt, eos)
            tok = select(scores, i).cpu()
            tok = torch.where(finished, torch.full_like(tok, eos), tok)
            finished |= tok == eos
            out[:, i] = tok
            nxt = tok.to(dev)
    return out, first


def _trimmed(ids, eos):
    done = (ids == eos).to(torch.int8).cummax(dim=1).values.bool().all(dim=0)
    return ids[:, : int(torch.nonzero(done)[0]) + 1] if bool(done.any()) else ids


def _selectors(V):
    T = 0.7
    return {"greedy": (dict(do_sample=False, temperature=T), lambda s, i: K.argmax_softmax(s, V, T)),
            "device-sampler": (dict(do_sample=True, temperature=T, top_k=20, top_p=0.9, seed=11),
                               lambda s, i: K.sample(s, V, T, top_k=20, top_p=0.9, min_p=0.0, seed=11, offset=i))}


CASES = [("last", "greedy", {}), ("text", "greedy", {}), ("long", "greedy", {}), ("last", "device-sampler", {}),
         ("text", "device-sampler", {}), ("text", "greedy", dict(repetition_penalty=1.2, no_repeat_ngram_size=2)),
         ("text", "device-sampler", dict(repetition_penalty=1.2, no_repeat_ngram_size=2)), ("text", "greedy", dict(decode_weights="mxfp8")),
         ("last", "greedy", dict(decode_weights="mxfp8")), ("text", "greedy", dict(sync_every=1)), ("long", "greedy", dict(sync_every=16))]


@pytest.mark.parametrize("kind,path,kw", CASES, ids=[f"{k}-{p}" + "".join(f"-{a}" for a in kw) for k, p, kw in CASES])
def test_generate_is_the_slow_loop(model, batch, kind, path, kw):
    m = model
    V, eos = m._llm_cfg.vocab_size, m.config.eos_token_idx
    gen, select = _selectors(V)[path]
    neg = _negative(batch, kind, eos)
    procs = (kw["repetition_penalty"], kw["no_repeat_ngram_size"], 0, ()) if "repetition_penalty" in kw else None
    try:
        ids = m.generate(batch, max_new_tokens=NEW, guidance_scale=3.0, negative_batch=neg, **gen, **kw)
        want, _ = _slow(m, batch, neg, 3.0, select, kw.get("decode_weights"), procs)
    finally:
        m.model.drop_decode_weights()
    assert ids.shape[0] == 2 and 1 <= ids.shape[1] <= NEW
    assert torch.equal(ids, _trimmed(want, eos)), (ids.tolist(), want.tolist())


def test_an_eos_reached_early_in_one_row(model, batch):
    """config.eos_token_idx set to an id the guided run emits in one row before the other ends: that pair keeps emitting eos (both of
    its rows are fed it), the other goes on, and the ids stay the slow loop's"""
    m = model
    V, eos0 = m._llm_cfg.vocab_size, m.config.eos_token_idx
    gen, select = _selectors(V)["greedy"]
    neg = _negative(batch, "text", eos0)
    base = m.generate(batch, max_new_tokens=NEW, guidance_scale=3.0, negative_batch=neg, **gen)
    cands = [int(t) for j in range(1, base.shape[1] - 2) for t in base[:, j] if int(t) != eos0]
    try:
        for e in dict.fromkeys(cands):
            m.config.eos_token_idx = e
            ids = m.generate(batch, max_new_tokens=NEW, guidance_scale=3.0, negative_batch=neg, sync_every=2, **gen)
            ends = sorted(ids[r].tolist().index(e) if e in ids[r].tolist() else NEW + 2 for r in range(2))
            if ends[0] + 2 <= min(ends[1], NEW - 1):
                want, _ = _slow(m, batch, neg, 3.0, select)
                assert torch.equal(ids, _trimmed(want, e)), (ids.tolist(), want.tolist())
                r = [ids[r].tolist().index(e) if e in ids[r].tolist() else NEW + 2 for r in range(2)].index(ends[0])
                assert bool((ids[r, ends[0]:] == e).all())
                return
    finally:
        m.config.eos_token_idx = eos0
    raise AssertionError(f"no id of {cands} ends one row early: {base.tolist()}")


def test_the_cases_cover_negatives_selectors_and_opt_ins():
    assert {c[0] for c in CASES} == {"last", "text", "long"} and {c[1] for c in CASES} == {"greedy", "device-sampler"}
    flat = [a for c in CASES for a in c[2].items()]
    assert ("repetition_penalty", 1.2) in flat and ("no_repeat_ngram_size", 2) in flat and ("decode_weights", "mxfp8") in flat
    assert ("sync_every", 1) in flat and ("sync_every", 16) in flat


# ---- the semantics, independent of the plumbing ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["last", "text", "long"])
def test_step_0_scores_are_the_formula_on_two_plain_forwards(model, batch, kind, monkeypatch):
    m, dev = model, model.device
    neg = _negative(batch, kind, m.config.eos_token_idx)
    seen = []
    real = K.cfg_combine
    monkeypatch.setattr(K, "cfg_combine", lambda x, st, s: seen.append(real(x, st, s).clone()) or seen[-1])
    m.generate(batch, max_new_tokens=1, do_sample=False, guidance_scale=3.0, negative_batch=neg)
    assert len(seen) == 1
    llm = m.model
    if neg is None:
        neg = dict(input_ids=batch["input_ids"][:, -1:], attention_mask=torch.ones(2, 1, dtype=torch.int64),
                   position_ids=torch.zeros(2, 1, dtype=torch.int64), processed_multimodal_inputs=NO_MM)
    rows = []
    with torch.no_grad():                                      # each batch alone, as generate prefills it without guidance
        for b in (batch, neg):
            S = b["input_ids"].shape[1]
            e = m.embed_modalities_with_text(b["input_ids"].to(dev), b["processed_multimodal_inputs"])
            rows.append(llm(past_key_values=llm.new_cache(2, S + 1), use_cache=True, inputs_embeds=e, logits_to_keep=1,
                            attention_mask=b["attention_mask"].to(dev), position_ids=b["position_ids"].to(dev)).logits[:, -1].cpu())
    cond, uncond = rows
    CC.check(f"step 0, {kind}", seen[0], cond, uncond, 3.0)


def test_it_does_something(model, batch, plain):
    """scale 3.0 against the image-less negative: on this fixture the fp32 CPU oracle (oracle/ref_cpu.py's decoder run once per half,
    the formula in torch) gives [[52, 52, ..], [20, 116, 20, 116, ..]] against plain greedy's [[22, 52, ..], [20, 122, 122, ..]]: row
    1 leaves its loop on 122 at the second token.  The scale was chosen there (1.5 changes row 1 alone, to a loop on 20)."""
    ids = model.generate(batch, max_new_tokens=NEW, do_sample=False, guidance_scale=3.0,
                         negative_batch=_negative(batch, "text", model.config.eos_token_idx))
    assert ids.shape != plain.shape or not torch.equal(ids, plain), ids.tolist()


# ---- off is off; one decoder call per step -----------------------------------------------------------------------------------------
class _Spies:
    def __init__(self, m, monkeypatch):
        self.combines, self.states, self.caches, self.decoder = [], [], [], []
        real_c, real_s, real_k, real_f = K.cfg_combine, K.GuidanceState, llm_mod.LayerKVCacheGuided, m.model.forward
        monkeypatch.setattr(K, "cfg_combine", lambda *a: self.combines.append(1) or real_c(*a))
        monkeypatch.setattr(K, "GuidanceState", lambda *a: self.states.append(1) or real_s(*a))
        monkeypatch.setattr(llm_mod, "LayerKVCacheGuided", lambda *a: self.caches.append(1) or real_k(*a))

        def forward(*a, **k):
            self.decoder.append(tuple(k["inputs_embeds"].shape[:2]))
            return real_f(*a, **k)

        monkeypatch.setattr(m.model, "forward", forward)


def test_off_is_off(model, batch, plain, monkeypatch):
    m = model
    sampled = m.generate(batch, max_new_tokens=NEW, temperature=0.8, top_k=20, seed=7)
    spies = _Spies(m, monkeypatch)
    for gs in (None, 1.0, 1):
        assert torch.equal(m.generate(batch, max_new_tokens=NEW, do_sample=False, guidance_scale=gs), plain)
        assert torch.equal(m.generate(batch, max_new_tokens=NEW, temperature=0.8, top_k=20, seed=7, guidance_scale=gs), sampled)
    assert spies.combines == [] and spies.states == [] and spies.caches == []
    assert all(rows == 2 for rows, _ in spies.decoder) and [s for _, s in spies.decoder].count(200) == 6      # one prefill per call


@pytest.mark.parametrize("kind", ["last", "text"])
def test_one_decoder_call_per_step_and_two_prefills(model, batch, monkeypatch, kind):
    m = model
    neg = _negative(batch, kind, m.config.eos_token_idx)
    spies = _Spies(m, monkeypatch)
    ids = m.generate(batch, max_new_tokens=NEW, do_sample=False, guidance_scale=3.0, negative_batch=neg, sync_every=1)
    Su = 1 if neg is None else neg["input_ids"].shape[1]
    n = len(spies.decoder) - 2
    assert spies.decoder[:2] == [(2, 200), (2, Su)] and spies.decoder[2:] == [(4, 1)] * n      # the unconditional prefill at ITS length
    assert ids.shape[1] - 1 <= n <= NEW - 1
    assert len(spies.combines) == n + 1 and spies.states == [1] and len(spies.caches) == m._llm_cfg.num_hidden_layers


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _refused(m, batch, match, **kw):
    """generate raises ValueError naming the argument before anything is encoded or decoded"""
    def boom(*a, **k):
        raise AssertionError("generate went on")
    m.model.forward = boom
    m.embed_modalities_with_text = boom
    try:
        with pytest.raises(ValueError, match=match):
            m.generate(batch, max_new_tokens=2, **kw)
    finally:
        del m.model.forward
        del m.embed_modalities_with_text


def test_generate_refuses(model, batch):
    m = model
    neg = _negative(batch, "text", m.config.eos_token_idx)
    for bad in (True, False, math.nan, math.inf, -math.inf, "3.0", [3.0]):
        _refused(m, batch, "guidance_scale", do_sample=False, guidance_scale=bad)
    for gs in (None, 1.0):                                      # a negative batch while guidance is off
        _refused(m, batch, "negative_batch.*guidance_scale", do_sample=False, guidance_scale=gs, negative_batch=neg)
    _refused(m, batch, "guidance_scale=3.0 with num_beams=2", do_sample=False, guidance_scale=3.0, num_beams=2)
    _refused(m, batch, "guidance_scale=3.0 with num_return_sequences=2", do_sample=True, guidance_scale=3.0, num_return_sequences=2)
    _refused(m, batch, "guidance_scale=3.0 with prompt_lookup_num_tokens=2", do_sample=False, guidance_scale=3.0, prompt_lookup_num_tokens=2)
    _refused(m, batch, "guidance_scale=3.0 with kv_cache='mxfp8'", do_sample=False, guidance_scale=3.0, kv_cache="mxfp8")
    one = {k: (v[:1] if torch.is_tensor(v) else v) for k, v in neg.items()}
    _refused(m, batch, "negative_batch of 1 rows with guidance_scale=3.0", do_sample=False, guidance_scale=3.0, negative_batch=one)
    _refused(m, batch, "negative_batch.*lacks position_ids", do_sample=False, guidance_scale=3.0,
             negative_batch={k: v for k, v in neg.items() if k != "position_ids"})
    nine = {k: (v[:1].repeat(9, 1) if torch.is_tensor(v) else v) for k, v in batch.items() if k != "processed_multimodal_inputs"}
    nine["processed_multimodal_inputs"] = NO_MM
    _refused(m, nine, "decode_weights='mxfp8' cannot be used: batch of 18", do_sample=False, guidance_scale=3.0, decode_weights="mxfp8")
    assert len(type(m).generate.__globals__["_REFUSALS"]) == 17
