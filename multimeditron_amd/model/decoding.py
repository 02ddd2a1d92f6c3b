"""The three decoding strategies behind MultiModalModelForCausalLM.generate(): Sampling, BeamSearch, PromptLookup.

The driver (MultiModalModelForCausalLM._decode) owns what every mode shares: the device setup, the first-use weight quantisation, the
cache, the prefill and every later decoder call, the look at a done flag every sync_every passes, the closing host copy and the eos
trim.  A strategy answers only what the driver asks, in this order:

    rows(B)                  how many rows a decoder pass after the prefill runs (generate's check of decode_weights)
    empty(B)                 the result of max_new_tokens <= 0
    cache_args(Sp, T)        (Smax, keyword arguments) of CausalLM.new_cache for a prompt of Sp positions and T new tokens
    begin(model, cache, input_ids, mask, T)      allocate the device state, once
    second_prefill()         asked once, between the prefill and consume(logits, 0): the arguments of a second prefill into the same
                             cache (the unconditional prompts of classifier-free guidance), or None; with one, consume(.., 0) gets the
                             pair (the prefill's logits, the second prefill's logits)
    consume(logits, i)       the logits of decoder pass i (0: the prefill) -> the selection, on the device
    done()                   the device flag the driver reads every sync_every passes
    feed(i)                  the arguments of decoder pass i >= 1: inputs_embeds, attention_mask, position_ids, and logits_to_keep=1
                             unless every position's logits are wanted
    finish()                 (ids, extra) on the host; extra is returned beside the ids when returns_extra is set
    trim_eos                 whether the driver cuts the ids behind the first column at which every row has emitted eos

Every pass but the prefill sits at "padded prompt length + i - 1" for every row (the reference's position quirk), or where the lookup's
device state says; the unconditional half of a guided pass sits at ITS OWN padded prompt length + i - 1."""
import torch

from .. import kernels as K


def _step_positions(rows, pos, device):
    return torch.full((rows, 1), pos, dtype=torch.long, device=device)


class Sampling:
    """Greedy (argmax(softmax(logits / T)), one kernel), torch.multinomial, or the device sampler: sampler = (top_k, top_p, min_p, seed)
    for the latter, else None.

    The reference synchronises with the host after EVERY token (`.cpu()`, `finished.all()`, model.py:618-625,637-638).  Here the chosen
    id, the eos bookkeeping and the next embedding lookup stay on the device (mm_decode_select + the embedding gather), so the host
    queues steps ahead of the GPU; it looks at `finished` only every `sync_every` tokens.  Steps issued past the point where every row
    had finished are cut off afterwards: the returned ids are exactly the reference's (same length, same values).

    samples = n > 1 (generate's num_return_sequences; opt-in; needs do_sample=True, greedy would return n equal rows): n sampled
    continuations of every prompt.  The modalities are encoded, spliced and prefilled ONCE per prompt, and the prompt's keys and values
    are stored once (LayerKVCacheShared: 2 Hkv D 2 (B Sp + B n max_new_tokens) bytes per layer instead of n copies of the prompt);
    the prefill's last-row logits are repeated n times and every later step runs B n rows, whose decode attention reads a
    prompt's keys once per 16 / (Hq / Hkv) samples (include/mm_hip.h: mm_attn_decode_shared -- the bits of the replicated
    batch's attention); the steps hand the PROMPT's mask to the cache (generated tokens are always visible).  Returns [B n, n_new]:
    row b n + j is sample j of prompt b (HF's order).  The device sampler draws
    with Philox offset = step and call = row b n + j; the torch.multinomial path draws per row; eos bookkeeping, sync_every,
    the early stop and the padded-length position quirk apply per row.  Composes with decode_weights (B n <= 16) and
    prefill_weights.  NOT with kv_cache="mxfp8" (a shared-prefix MXFP8 cache is out of scope: ValueError).  A model that
    cannot use it -- not bf16, head_dim other than 128, a number of query heads per key/value head other than 1, 2 or 4 --
    raises ValueError before the prefill (CausalLM.samples_ok).  n = 1 is the path above, untouched.

    processors = (repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppressed ids), checked by generate, else None
    (repetition_penalty= / no_repeat_ngram_size= / min_new_tokens= / suppress_tokens=: opt-in, each on its own): transformers'
    RepetitionPenalty -> NoRepeatNGram -> MinNewTokensLength -> SuppressTokens logits processors, applied in that order to the
    fp32 scores of every step by ONE kernel (include/mm_hip.h: mm_logits_process) between lm_head and the selection; greedy,
    torch.multinomial and the device sampler then select from its fp32 output unchanged.  The history of a row -- what the
    penalty and the n-gram ban look at -- lives on the device: the prompt's ids first, then every emitted id (the eos ids a
    finished row keeps emitting included), appended by the kernel from next_ids; the host sees no token.  As in transformers'
    decoder-only generate the PROMPT counts, placeholder ids of spliced modalities like any id; the one deviation: positions whose
    attention_mask is 0 (pads) do not count (a pad == eos tokenizer would otherwise penalise eos on every padded row).
    repetition_penalty: a finite number > 0 (None or 1.0: off); no_repeat_ngram_size, min_new_tokens: ints >= 0 (None or 0: off;
    min_new_tokens bans config.eos_token_idx while step < min_new_tokens); suppress_tokens: ids in [0, vocab_size) that are never
    chosen, e.g. the attachment placeholder and pad ids (None or empty: off).  Compose with decode_weights, kv_cache,
    prefill_weights, num_return_sequences (every sample row keeps its own history) and every sampler path.  NOT with num_beams > 1
    (processors inside beam search act on log-probabilities inside mm_beam_step: out of scope, ValueError).  A bad value raises
    ValueError before the modalities are encoded.  With all four off nothing changes: no launch, no buffer, the same ids.

    guidance = (scale, negative_batch or None), checked by generate, else None (guidance_scale= / negative_batch=: opt-in):
    classifier-free guidance, transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor -- the FIRST processor of HF's chain --
    with both halves in ONE decoder pass.  Row b of the batch is paired with an unconditional row: row b of negative_batch (a collated
    batch of the same B rows with its own input_ids / attention_mask / position_ids / processed_multimodal_inputs, e.g. the same
    conversation without its image), or, without one, HF's default: the last id of the prompt as one position (mask 1, position 0).
    The prefill is followed by a second prefill of the B unconditional prompts at their OWN padded length Su into rows [B, 2 B) of a
    LayerKVCacheGuided; every later pass runs 2 B rows x 1 on one stream of the weights.  Per step, in fp32, scores =
    log_softmax(x_u) + scale * (log_softmax(x_c) - log_softmax(x_u)) (include/mm_hip.h: mm_cfg_combine, two short launches) take the
    place of the logits for everything that follows: the four processors (their history is the CONDITIONAL prompt's, as HF passes
    input_ids) and greedy / torch.multinomial / the device sampler on B fp32 rows.  Both rows of a pair are fed the SAME chosen id;
    eos bookkeeping, sync_every, the early stop and the returned [B, n_new] ids are per pair.  The conditional rows step at Sc + i - 1
    and the unconditional ones at Su + i - 1: what generate would use for each batch alone.  The unconditional rows stream Sp + i key
    slots (Sp = max(Sc, Su)) although only Su + i are live.  Composes with decode_weights (2 B <= 16 rows), prefill_weights (both
    prefills), the processors and every sampler path.  NOT with num_beams > 1, num_return_sequences > 1, prompt_lookup_num_tokens
    or kv_cache="mxfp8" (a second multi-token store into an MXFP8 cache is what LayerKVCacheMX8.accept refuses): ValueError before
    the modalities are encoded.  guidance_scale None or 1.0 is off: no launch, no buffer, no second prefill, the same ids."""
    returns_extra, trim_eos = False, True

    def __init__(self, temperature, do_sample, sampler=None, samples=1, kv_cache=None, processors=None, guidance=None):
        self.temperature, self.do_sample, self.sampler = max(temperature, 1e-6), do_sample, sampler
        self.samples, self.kv_cache, self.processors, self.guidance = samples, kv_cache, processors, guidance
        self.negative = None

    def rows(self, B):
        return B * self.samples * (2 if self.guidance is not None else 1)

    def empty(self, B):
        return torch.empty((B * self.samples, 0), dtype=torch.int64), None

    def cache_args(self, Sp, T):
        if self.guidance is not None:
            neg = self.guidance[1]
            Sp = max(Sp, 1 if neg is None else int(neg["input_ids"].shape[1]))
            return Sp + T, dict(guided=True, prompt_len=Sp)
        return Sp + T, (dict(samples=self.samples, prompt_len=Sp) if self.samples > 1 else dict(kv_cache=self.kv_cache))

    def _begin_guidance(self, model, input_ids, mask, T):
        """The unconditional half: its prefill's arguments, the mask [2 B, Sp + T] of the right-aligned halves, the positions."""
        dev, (B, Sc), neg = input_ids.device, mask.shape, self.guidance[1]
        if neg is None:                               # HF's default: the last id of the prompt, as one position
            nmask, npos = torch.ones((B, 1), dtype=mask.dtype, device=dev), torch.zeros((B, 1), dtype=torch.long, device=dev)
            embeds = self.emb(input_ids[:, -1:])
        else:
            nmask, npos = neg["attention_mask"].to(dev), neg["position_ids"].to(dev)
            embeds = model.embed_modalities_with_text(neg["input_ids"].to(dev), neg["processed_multimodal_inputs"])
        Su = nmask.shape[1]
        self.negative = dict(inputs_embeds=embeds, attention_mask=nmask, position_ids=npos, logits_to_keep=1)
        self.Sp = max(Sc, Su)
        self.mask = torch.zeros((2 * B, self.Sp + T), dtype=mask.dtype, device=dev)
        self.mask[:, self.Sp:] = 1
        self.mask[:B, self.Sp - Sc:self.Sp] = mask
        self.mask[B:, self.Sp - Su:self.Sp] = nmask
        self.pos = torch.cat([torch.full((B, 1), Sc, dtype=torch.long, device=dev), torch.full((B, 1), Su, dtype=torch.long, device=dev)])
        self.gs = K.GuidanceState(B, self.V, dev)

    def second_prefill(self):
        return self.negative

    def begin(self, model, cache, input_ids, mask, T):
        # device-resident loop state (plumbing): the growing mask is a view of one preallocated buffer
        dev, (B, self.Sp) = input_ids.device, mask.shape
        self.R = R = B * self.samples              # the rows of every buffer below and of every step after the prefill
        self.V, self.eos, self.emb = model._llm_cfg.vocab_size, model.config.eos_token_idx, model.model.get_input_embeddings()
        self.mask = mask
        if self.guidance is not None:
            self._begin_guidance(model, input_ids, mask, T)
        elif self.samples == 1:
            self.mask = torch.ones((B, self.Sp + T), dtype=mask.dtype, device=dev)
            self.mask[:, :self.Sp] = mask
        self.out_ids = torch.full((R, T), self.eos, dtype=torch.int64, device=dev)
        self.finished = torch.zeros(R, dtype=torch.uint8, device=dev)
        self.next_ids = torch.empty(R, dtype=torch.int64, device=dev)
        self.ws = K.sample_ws(R, self.V, dev) if self.sampler is not None else None       # once per call
        self.tok_buf = torch.empty(R, dtype=torch.int64, device=dev) if self.sampler is not None else None
        self.lp = None
        if self.processors is not None:
            self.lp = K.LogitsState(R, self.V, dev, *self.processors, prompt_ids=input_ids, prompt_mask=mask, samples=self.samples, room=T)

    def consume(self, logits, i):
        if self.guidance is not None:                     # fp32 scores of the B pairs take the place of the logits
            both = torch.cat([l[:, -1, :] for l in logits]) if i == 0 else logits[:, -1, :]     # plumbing: the two prefills' last rows
            logits2d = K.cfg_combine(both, self.gs, self.guidance[0])
        else:
            logits2d = logits[:, -1, :]                   # [rows, V] view, stride padded
        if self.samples > 1 and i == 0:
            logits2d = logits2d.repeat_interleave(self.samples, dim=0)      # plumbing: sample j of prompt b is row b n + j
        if self.lp is not None:
            logits2d = K.logits_process(logits2d, self.lp, i, self.next_ids, self.eos)    # fp32 scores; the history takes next_ids in
        if self.sampler is not None:
            k_, p_, mp_, sd_ = self.sampler
            tok = K.sample(logits2d, self.V, self.temperature, top_k=k_, top_p=p_, min_p=mp_, seed=sd_, offset=i, ws=self.ws, out=self.tok_buf)
        elif self.do_sample:
            tok = torch.multinomial(torch.softmax(logits2d.float() / self.temperature, dim=-1), num_samples=1).view(self.R)
        else:
            tok = K.argmax_softmax(logits2d, self.V, self.temperature)
        K.decode_select(tok, self.finished, self.eos, self.out_ids, i, self.next_ids)
        self.steps = i + 1

    def done(self):
        return self.finished.all()

    def feed(self, i):
        if self.guidance is not None:                     # both rows of a pair take the chosen id, each half at its own position
            return dict(inputs_embeds=self.emb(self.next_ids.repeat(2).view(2 * self.R, 1)), position_ids=self.pos + (i - 1),
                        logits_to_keep=1, attention_mask=self.mask[:, : self.Sp + i])
        nxt = self.emb(self.next_ids.view(self.R, 1))
        return dict(inputs_embeds=nxt, position_ids=_step_positions(self.R, self.Sp + i - 1, nxt.device), logits_to_keep=1,
                    attention_mask=self.mask[:, : self.Sp + i] if self.samples == 1 else self.mask)

    def finish(self):
        return self.out_ids[:, :self.steps].cpu(), None


class BeamSearch:
    """num_beams=n > 1 (opt-in; needs do_sample=False): beam search as transformers' generate(num_beams=n, do_sample=False,
    length_penalty=, early_stopping=) with one eos token and no logits processors; the rules are written out in
    include/mm_hip.h (mm_beam_step).  One prefill per prompt into a LayerKVCacheBeam (the prompt's keys once, as for samples), then
    B n rows per step; the selection over a prompt's n V continuations, the finished hypotheses and the stopping flags live on the
    device (mm_beam_step reads the prefill's B rows of logits at step 0 and B n rows afterwards, and hands back the next ids -- the next
    embedding lookup -- and the ancestor table of the coming step), and a beam continues another row's suffix through an int32 ancestor
    table instead of a reordered cache (mm_attn_decode_beam).  The host looks at the device's done flag every `sync_every` steps; steps
    issued past it change nothing.  Positions keep the padded-length quirk and the cache gets the PROMPT's mask.
    early_stopping in {False, True, "never"} and length_penalty have HF's meaning; temperature is ignored.  Returns
    [B num_return_sequences, n_out] (num_return_sequences <= n, default 1): row b nrs + k is prompt b's k-th best finished
    hypothesis, eos included and filled with eos behind its end, n_out the longest returned one; with return_beam_scores=True
    (ids, scores), scores [B nrs] fp32 = sum of log-probabilities / length ** length_penalty, descending per prompt.
    Composes with decode_weights (B n <= 16) and prefill_weights.  ValueError before the modalities are encoded for: num_beams
    outside [1, 16], do_sample=True, any of top_k / top_p / min_p / seed / generator, kv_cache="mxfp8", num_return_sequences >
    num_beams, a length_penalty that is not finite, another early_stopping, a vocabulary below 2 n, and a model samples_ok
    refuses.  num_beams = 1 is Sampling, untouched."""
    trim_eos = False

    def __init__(self, n, nrs, length_penalty, early_stopping, return_scores):
        self.n, self.nrs, self.length_penalty, self.early_stopping, self.returns_extra = n, nrs, length_penalty, early_stopping, return_scores

    def rows(self, B):
        return B * self.n

    def second_prefill(self):
        return None

    def empty(self, B):
        return torch.empty((B * self.nrs, 0), dtype=torch.int64), torch.zeros(B * self.nrs, dtype=torch.float32)

    def cache_args(self, Sp, T):
        return Sp + T, dict(beams=self.n, prompt_len=Sp)

    def begin(self, model, cache, input_ids, mask, T):
        (B, self.Sp), self.mask, self.tables = mask.shape, mask, cache[0].tables
        self.R, self.eos, self.emb = B * self.n, model.config.eos_token_idx, model.model.get_input_embeddings()
        self.st = K.BeamState(B, self.n, T, model._llm_cfg.vocab_size, input_ids.device)

    def consume(self, logits, i):
        self.next_ids = K.beam_step(logits[:, -1, :], self.st, i, self.eos, self.length_penalty, self.early_stopping)

    def done(self):
        return self.st.done

    def feed(self, i):
        nxt = self.emb(self.next_ids.view(self.R, 1))
        self.tables.current = self.st.table(i)
        return dict(inputs_embeds=nxt, attention_mask=self.mask, position_ids=_step_positions(self.R, self.Sp + i - 1, nxt.device),
                    logits_to_keep=1)

    def finish(self):
        ids, scores, lens = K.beam_finish(self.st, self.nrs, self.eos)
        return ids[:, :int(lens.max().item())].cpu(), scores.cpu()


class PromptLookup:
    """prompt_lookup_num_tokens=k (opt-in; greedy: needs do_sample=False): prompt-lookup speculative decoding, transformers'
    generate(prompt_lookup_num_tokens=k, max_matching_ngram_size=G) for B rows at once.  Each iteration proposes up to k next
    tokens per row by matching the row's last n-gram (n <= G, default 2; the first match of the longest n) in its own visible
    prompt and output (include/mm_hip.h: mm_lookup_draft -- PromptLookupCandidateGenerator.get_candidates per row), runs ONE
    decoder pass over k + 1 positions per row -- B (k + 1) <= 16 rows, the rows a weight-streaming launch has to spare -- and keeps
    every proposed token the model would have chosen itself (mm_lookup_accept), so the ids are plain greedy decoding's up to the
    rounding of a differently sliced attention sum.  Rows advance by different amounts; their positions, histories and the done
    flag live on the device and the host reads only that flag, every `sync_every` iterations.  As everywhere here the prompt's
    masked positions do not count as history.  Returns the ids as Sampling does; with return_lookup_stats=True (ids, stats), stats int32
    [B, 2] on the CPU: verify steps run (the prefill's included) and draft tokens accepted, per row.  Composes with
    decode_weights (the verify step reads the copies) and prefill_weights.  Out of scope, ValueError before the modalities are
    encoded: sampling (do_sample=True, top_k / top_p / min_p / seed / generator), logits processors, num_beams > 1,
    num_return_sequences > 1 (shared-prefix samples), kv_cache="mxfp8", k not an int >= 1, B (k + 1) > 16, a model
    CausalLM.lookup_ok refuses, and return_lookup_stats / max_matching_ngram_size without k.  Not here either: a draft model
    (assistant_model), adaptive k, the append fused into the RoPE pass, tuned slice counts of the verify attention.  With
    prompt_lookup_num_tokens=None nothing changes: no launch, no buffer, the same ids.

    The prefill runs as Sampling's into a LayerKVCacheLookup with room for k slots behind the last id; its token goes through
    mm_lookup_accept as a verify step without drafts, so count, finished, the history and base (seq_length - 1 -> seq_length: the
    "padded prompt length + i - 1" position and cache slot of the first generated token) start out the way later steps update
    them.  An iteration is mm_lookup_draft -> embedding gather -> one decoder pass over k + 1 positions per row (CausalLM.forward's
    verify step) with lm_head on all B (k + 1) rows -> the selector plain greedy uses, at the caller's temperature ->
    mm_lookup_accept.  At most max_new_tokens accept calls (every one emits at least one id per active row); iterations issued
    after done change nothing."""
    trim_eos = True

    def __init__(self, k, G, temperature, return_stats):
        self.k, self.G, self.temperature, self.returns_extra = k, G, max(temperature, 1e-6), return_stats

    def rows(self, B):
        return B * (self.k + 1)

    def second_prefill(self):
        return None

    def empty(self, B):
        return torch.empty((B, 0), dtype=torch.int64), torch.zeros((B, 2), dtype=torch.int32)

    def cache_args(self, Sp, T):
        return Sp + T + self.k, dict(lookup=self.k)

    def begin(self, model, cache, input_ids, mask, T):
        (self.B, self.Sp), self.T, self.V = mask.shape, T, model._llm_cfg.vocab_size
        self.emb, self.shared = model.model.get_input_embeddings(), cache[0].shared
        self.st = K.LookupState(input_ids, mask, self.k, self.G, T, model.config.eos_token_idx, self.Sp - 1)
        self.shared.base = self.st.base
        self.mask = mask.to(torch.int64).contiguous()

    def consume(self, logits, i):
        if i == 0:
            K.lookup_accept(self.st, K.argmax_softmax(logits[:, -1, :], self.V, self.temperature), 1)
        else:
            K.lookup_accept(self.st, K.argmax_softmax(logits.reshape(self.B * (self.k + 1), self.V), self.V, self.temperature))

    def done(self):
        return self.st.done

    def feed(self, i):
        self.shared.bound = min(self.Sp + (i - 1) * (self.k + 1), self.Sp + self.T - 1)      # base[b] <= bound, known here
        ids, pos = K.lookup_draft(self.st)
        return dict(inputs_embeds=self.emb(ids), attention_mask=self.mask, position_ids=pos)

    def finish(self):
        ids, stats, count = self.st.out.cpu(), self.st.stats.cpu(), self.st.count.cpu()
        return ids[:, : int(count.max())], stats
