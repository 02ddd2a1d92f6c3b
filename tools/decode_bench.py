#!/usr/bin/env python3
"""generate() timing on the 8B workload: prefill and per-token decode (run on the GPU box).
   python tools/decode_bench.py [B] [S] [new_tokens] [--sample top_p=0.95,T=0.7] [--decode-weights mxfp8] [--kv-cache mxfp8]
                                [--prefill-weights mxfp8] [--samples n] [--beams n]
                                [--processors repetition_penalty=1.2,no_repeat_ngram_size=3] [--lookup K[,G]]
                                [--guidance S[,negative=last|text]]
--sample: the device sampler (generate(do_sample=True, ...)) with the listed settings (T, top_k, top_p, min_p, seed) instead of
the greedy selection.  --decode-weights mxfp8: the decode steps stream the weight-only MXFP8 copies (generate(decode_weights=...));
the copies are made by the warm-up call, outside the timed ones.  --kv-cache mxfp8: the KV cache is kept in MXFP8
(generate(kv_cache=...)).  --prefill-weights mxfp8: the prefill runs its decoder linears as MXFP8 x MXFP8 GEMMs
(generate(prefill_weights=...)); the first step alone (max_new_tokens = 1: the prefill and one token choice) is then timed for BOTH
settings in this process, best of three after a warm-up each, before the usual line.  The KV bytes a decode step reads per token
(every layer's K and V of B x S positions) are printed.
--samples n: in this one process, (i) generate(num_return_sequences=n) on the B prompts against (ii) the existing path on the prompts
repeated n times (a batch of B n rows), alternating, best of three each after a warm-up: prefill + 1 token, ms/token and the bytes of
the KV cache each allocates; then the decode-attention launch alone at the last step's lengths, mm_attn_decode_shared on the shared
cache against mm_attn_decode on B n rows, over 16 layers' caches.  Sampled (T = 1, seed 0 unless --sample says otherwise).  The other
flags apply to both sides (--kv-cache is refused by generate with n > 1).
--beams n: in this one process, (i) generate(num_beams=n, do_sample=False) against (ii) generate(num_return_sequences=n) sampled at
T = 1, seed 0 -- the closest existing path: the same B n rows over one shared prompt cache, so the difference is the price of the
selection and of the ancestor table -- alternating, best of three each after a warm-up; then mm_attn_decode_beam under an identity
table against mm_attn_decode_shared at the last step's lengths, and the launches of one mm_beam_step against mm_sample (top_k = 50,
top_p = 0.95) on 16 rows of the model's vocabulary.
--processors k=v,...: in this one process, generate with the listed logits processors (repetition_penalty, no_repeat_ngram_size,
min_new_tokens, suppress_tokens=a+b+c) against the same call without them, alternating, best of three each after a warm-up:
prefill + 1 token and ms/token of both and the difference (one mm_logits_process launch per step, and the selection reading fp32
scores instead of bf16 logits).  The other flags apply to both sides.
--lookup K[,G]: in this one process, greedy generate(prompt_lookup_num_tokens=K, max_matching_ngram_size=G) against the same call
without the lookup, alternating, best of three each after a warm-up: ms per verify iteration against ms per plain step (their ratio
is the number that transfers), accepted drafts per iteration and tokens/s (this model's weights are random: its acceptance rate is
whatever its loops give); then the launches alone -- mm_attn_decode_verify against mm_attn_decode over 16 layers' caches, and
mm_lookup_draft / mm_kv_append_at / mm_lookup_accept.  --decode-weights and --prefill-weights apply to both sides.
--guidance S[,negative=last|text]: in this one process, greedy generate(guidance_scale=S) -- the conditional and the unconditional
rows in ONE decoder pass of 2 B rows -- against plain greedy at B rows and against the two-pass form it replaces, alternating, best
of three each after a warm-up.  negative=last (default): HF's default unconditional prompt, the last id as one position; negative=text:
the batch without its image spans (negative_batch=).  The two-pass form is a plain step of the B prompts plus a plain step of the B
unconditional prompts per token (each timed as a plain generate of that batch alone), reported as `2 x plain`; prefill + 1 token of
all three.  --decode-weights and --prefill-weights apply to every side."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from multimeditron_amd.model.model import MultimodalConfig, MultiModalModelForCausalLM
from multimeditron_amd.model.modalities import ImageConfig
from multimeditron_amd.model.presets import resolve_llm_config, resolve_vision_config

SAMPLE = None
if "--sample" in sys.argv:
    i = sys.argv.index("--sample")
    SAMPLE = {}
    for kv in sys.argv[i + 1].split(","):
        k, val = kv.split("=")
        SAMPLE[k] = int(val) if k in ("top_k", "seed") else float(val)
    del sys.argv[i:i + 2]
DW = None
if "--decode-weights" in sys.argv:
    i = sys.argv.index("--decode-weights")
    DW = sys.argv[i + 1]
    del sys.argv[i:i + 2]
KV = None
if "--kv-cache" in sys.argv:
    i = sys.argv.index("--kv-cache")
    KV = sys.argv[i + 1]
    del sys.argv[i:i + 2]
PW = None
if "--prefill-weights" in sys.argv:
    i = sys.argv.index("--prefill-weights")
    PW = sys.argv[i + 1]
    del sys.argv[i:i + 2]
NS = 1
if "--samples" in sys.argv:
    i = sys.argv.index("--samples")
    NS = int(sys.argv[i + 1])
    del sys.argv[i:i + 2]
    if SAMPLE is None:
        SAMPLE = {"T": 1.0, "seed": 0}
NB = 1
if "--beams" in sys.argv:
    i = sys.argv.index("--beams")
    NB = int(sys.argv[i + 1])
    del sys.argv[i:i + 2]
PROC = None
if "--processors" in sys.argv:
    i = sys.argv.index("--processors")
    PROC = {}
    for kv in sys.argv[i + 1].split(","):
        k, val = kv.split("=")
        PROC[k] = float(val) if k == "repetition_penalty" else [int(t) for t in val.split("+")] if k == "suppress_tokens" else int(val)
    del sys.argv[i:i + 2]
LOOKUP = None
if "--lookup" in sys.argv:
    i = sys.argv.index("--lookup")
    LOOKUP = [int(t) for t in sys.argv[i + 1].split(",")]
    del sys.argv[i:i + 2]
GUIDE = None
if "--guidance" in sys.argv:
    i = sys.argv.index("--guidance")
    parts = sys.argv[i + 1].split(",")
    GUIDE = (float(parts[0]), dict(kv.split("=") for kv in parts[1:]).get("negative", "last"))
    assert GUIDE[1] in ("last", "text"), GUIDE
    del sys.argv[i:i + 2]
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
S = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
N = int(sys.argv[3]) if len(sys.argv) > 3 else 33
llm_name, clip_name = "meta-llama/Llama-3.1-8B-Instruct", "openai/clip-vit-large-patch14"
llm, vis = resolve_llm_config(llm_name), resolve_vision_config(clip_name)
vocab = llm["vocab_size"] + 2
torch.manual_seed(0)
cfg = MultimodalConfig(vocab_size=vocab, modalities=[ImageConfig(hidden_size=llm["hidden_size"], clip_name=clip_name)],
                       llm_path=llm_name, dtype="bfloat16", eos_token_idx=vocab + 5, hidden_size=llm["hidden_size"])   # eos never hit
model = MultiModalModelForCausalLM(cfg, device="cuda")
model.pack_parameters()
batch, _ = bench.synthetic_batch(B, S, 1, 256, vocab, (llm["vocab_size"], llm["vocab_size"] + 1, 128002), 7, "cuda", 224)
batch["attention_mask"] = torch.ones(B, S, dtype=torch.long, device="cuda")


def repeated(batch, n):
    """the batch with every prompt n times in a row (row b n + j = prompt b): what a caller without num_return_sequences builds"""
    mm = batch["processed_multimodal_inputs"]
    P = mm["token_range"]["image"].numel() // B
    return dict(input_ids=batch["input_ids"].repeat_interleave(n, 0), position_ids=batch["position_ids"].repeat_interleave(n, 0),
                attention_mask=batch["attention_mask"].repeat_interleave(n, 0), labels=None,
                processed_multimodal_inputs={"batch_idx": {"image": torch.arange(B * n, device="cuda").repeat_interleave(P)},
                                             "token_range": {"image": mm["token_range"]["image"].view(B, P).repeat_interleave(n, 0).reshape(-1)},
                                             "stacked": {"image": mm["stacked"]["image"].repeat_interleave(n, 0)}})


def compare_samples(n):
    from multimeditron_amd import kernels as K
    kw = dict(SAMPLE)
    T = kw.pop("T", 1.0)
    kw.setdefault("seed", 0)
    if DW:
        kw["decode_weights"] = DW
    if PW:
        kw["prefill_weights"] = PW
    rep = repeated(batch, n)
    made = []
    new_cache = model.model.new_cache
    model.model.new_cache = lambda *a, **k: made.append(new_cache(*a, **k)) or made[-1]

    def go(shared, new):
        del made[:]
        torch.cuda.synchronize()
        t = time.perf_counter()
        ids = model.generate(batch, max_new_tokens=new, temperature=T, num_return_sequences=n, **kw) if shared else \
            model.generate(rep, max_new_tokens=new, temperature=T, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        nbytes = sum(t_.numel() * t_.element_size() for c in made[0] for t_ in vars(c).values() if torch.is_tensor(t_))
        del made[:]
        return dt, ids, nbytes

    res = {}
    for shared in (True, False):
        go(shared, 2)                                      # warm-up (and the MXFP8 copies, if asked for)
    t1, tn = {True: [], False: []}, {True: [], False: []}
    for _ in range(3):                                     # alternating
        for shared in (True, False):
            t1[shared].append(go(shared, 1)[0])
            dt, ids, nbytes = go(shared, N)
            tn[shared].append(dt)
            res[shared] = (tuple(ids.shape), nbytes)
    for shared in (True, False):
        a, b = min(t1[shared]), min(tn[shared])
        name = f"num_return_sequences={n} on {B} prompts" if shared else f"{B} prompts repeated {n} times ({B * n} rows)"
        print(f"{name}: prefill+1 token {a * 1e3:.1f} ms; decode {(b - a) / (N - 1) * 1e3:.2f} ms/token (all runs "
              f"{', '.join(f'{(y - x) / (N - 1) * 1e3:.2f}' for x, y in zip(t1[shared], tn[shared]))}); KV cache {res[shared][1] / 1e9:.3f} GB allocated; "
              f"ids {res[shared][0]}", flush=True)
    model.model.new_cache = new_cache
    # the decode-attention launch alone, at the last step's lengths
    lc = model.model.config
    Hq, Hkv, D, L, Ss = lc.num_attention_heads, lc.num_key_value_heads, lc.head_dim, 16, N - 1
    bf = torch.bfloat16
    q = torch.randn(B * n, Hq, D, device="cuda", dtype=bf)
    kp = [torch.randn(B, S, Hkv, D, device="cuda", dtype=bf) for _ in range(2 * L)]
    ks = [torch.randn(B * n, N, Hkv, D, device="cuda", dtype=bf) for _ in range(2 * L)]
    kr = [torch.randn(B * n, S + N, Hkv, D, device="cuda", dtype=bf) for _ in range(2 * L)]

    def timed(name, fn, nbytes, reps=6):
        for i in range(L):
            fn(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            for i in range(L):
                fn(i)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / (reps * L)
        print(f"{name:58s} {us:7.1f} us/launch   {nbytes / 1e6:6.1f} MB of keys and values   {nbytes / us / 1e6:5.2f} TB/s", flush=True)

    row = 2 * Hkv * D * 2
    for _ in range(2):
        timed(f"attention, shared prefix ({B} x {S} + {B * n} x {Ss} keys)",
              lambda i: K.attn_decode_shared(q, kp[2 * i], kp[2 * i + 1], ks[2 * i][:, :Ss], ks[2 * i + 1][:, :Ss], n, None, D ** -0.5),
              (B * S + B * n * Ss) * row)
        timed(f"attention, replicated ({B * n} x {S + Ss} keys)",
              lambda i: K.attn_decode(q, kr[2 * i][:, :S + Ss], kr[2 * i + 1][:, :S + Ss], None, D ** -0.5), B * n * (S + Ss) * row)


def compare_beams(n):
    from multimeditron_amd import kernels as K
    kw = {}
    if DW:
        kw["decode_weights"] = DW
    if PW:
        kw["prefill_weights"] = PW

    def go(beams, new):
        torch.cuda.synchronize()
        t = time.perf_counter()
        ids = model.generate(batch, max_new_tokens=new, do_sample=False, num_beams=n, num_return_sequences=n, **kw) if beams else \
            model.generate(batch, max_new_tokens=new, temperature=1.0, seed=0, num_return_sequences=n, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t, ids

    for beams in (True, False):
        go(beams, 2)                                       # warm-up (and the MXFP8 copies, if asked for)
    t1, tn, shape = {True: [], False: []}, {True: [], False: []}, {}
    for _ in range(3):                                     # alternating
        for beams in (True, False):
            t1[beams].append(go(beams, 1)[0])
            dt, ids = go(beams, N)
            tn[beams].append(dt)
            shape[beams] = tuple(ids.shape)
    for beams in (True, False):
        a, b = min(t1[beams]), min(tn[beams])
        name = f"num_beams={n} on {B} prompts" if beams else f"num_return_sequences={n} on {B} prompts (sampled)"
        print(f"{name}: prefill+1 token {a * 1e3:.1f} ms; decode {(b - a) / (N - 1) * 1e3:.2f} ms/token (all runs "
              f"{', '.join(f'{(y - x) / (N - 1) * 1e3:.2f}' for x, y in zip(t1[beams], tn[beams]))}); ids {shape[beams]}", flush=True)
    lc = model.model.config
    Hq, Hkv, D, L, Ss = lc.num_attention_heads, lc.num_key_value_heads, lc.head_dim, 16, N - 1
    bf = torch.bfloat16
    q = torch.randn(B * n, Hq, D, device="cuda", dtype=bf)
    kp = [torch.randn(B, S, Hkv, D, device="cuda", dtype=bf) for _ in range(2 * L)]
    ks = [torch.randn(B * n, N, Hkv, D, device="cuda", dtype=bf) for _ in range(2 * L)]
    ident = torch.arange(B * n, dtype=torch.int32, device="cuda")[None, :].expand(N, B * n).contiguous()

    def timed(name, fn, reps=6, per=L):
        for i in range(per):
            fn(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            for i in range(per):
                fn(i)
        e1.record()
        torch.cuda.synchronize()
        print(f"{name:66s} {e0.elapsed_time(e1) * 1e3 / (reps * per):7.1f} us/call", flush=True)

    for _ in range(2):
        timed(f"mm_attn_decode_beam, identity table ({B} x {S} + {B * n} x {Ss} keys)",
              lambda i: K.attn_decode_beam(q, kp[2 * i], kp[2 * i + 1], ks[2 * i][:, :Ss], ks[2 * i + 1][:, :Ss], n, None, D ** -0.5, ident))
        timed(f"mm_attn_decode_shared ({B} x {S} + {B * n} x {Ss} keys)",
              lambda i: K.attn_decode_shared(q, kp[2 * i], kp[2 * i + 1], ks[2 * i][:, :Ss], ks[2 * i + 1][:, :Ss], n, None, D ** -0.5))
    V = lc.vocab_size
    rows = 16
    logits = (3 * torch.randn(rows, V + 6, device="cuda")).to(bf)[:, :V]
    for nb in sorted({n, 16}):
        Bq = rows // nb
        st = K.BeamState(Bq, nb, 64, V, "cuda")
        K.beam_step(logits[:Bq], st, 0, V + 5, 1.0, False)
        timed(f"mm_beam_step, {Bq} prompts x {nb} beams = {Bq * nb} rows of {V} (3 launches)",
              lambda i: K.beam_step(logits[:Bq * nb], st, 1 + i % 8, V + 5, 1.0, False), per=8)
    ws = K.sample_ws(rows, V, "cuda")
    timed(f"mm_sample top_k=50 top_p=0.95, {rows} rows of {V} (9 launches)",
          lambda i: K.sample(logits, V, 1.0, top_k=50, top_p=0.95, seed=0, offset=i, ws=ws), per=8)
    timed(f"mm_sample plain, {rows} rows of {V} (3 launches)", lambda i: K.sample(logits, V, 1.0, seed=0, offset=i, ws=ws), per=8)


def run(n, pw="same", proc=None):
    torch.cuda.synchronize()
    t = time.perf_counter()
    dw = {"decode_weights": DW} if DW else {}
    pw = PW if pw == "same" else pw
    if pw:
        dw["prefill_weights"] = pw
    if KV:
        dw["kv_cache"] = KV
    if proc:
        dw.update(proc)
    if SAMPLE is None:
        ids = model.generate(batch, max_new_tokens=n, temperature=0.1, do_sample=False, **dw)
    else:
        kw = dict(SAMPLE)
        T = kw.pop("T", 1.0)
        kw.setdefault("seed", 0)
        ids = model.generate(batch, max_new_tokens=n, temperature=T, do_sample=True, **kw, **dw)
    torch.cuda.synchronize()
    return time.perf_counter() - t, ids


def compare_processors(proc):
    for on in (True, False):
        run(2, proc=proc if on else None)                  # warm-up (and the MXFP8 copies, if asked for)
    t1, tn = {True: [], False: []}, {True: [], False: []}
    for _ in range(3):                                     # alternating
        for on in (True, False):
            t1[on].append(run(1, proc=proc if on else None)[0])
            tn[on].append(run(N, proc=proc if on else None)[0])
    per = {}
    for on in (True, False):
        a, b = min(t1[on]), min(tn[on])
        per[on] = (b - a) / (N - 1) * 1e3
        print(f"B={B} S={S} processors {proc if on else 'off'}: prefill+1 token {a * 1e3:.1f} ms; decode {per[on]:.3f} ms/token (all runs "
              f"{', '.join(f'{(y - x) / (N - 1) * 1e3:.3f}' for x, y in zip(t1[on], tn[on]))})", flush=True)
    print(f"processors on - off: {(per[True] - per[False]) * 1e3:+.1f} us/token ({(per[True] / per[False] - 1) * 100:+.2f} %)", flush=True)


def compare_lookup(k, G=2):
    from multimeditron_amd import kernels as K
    kw = {"decode_weights": DW} if DW else {}
    if PW:
        kw["prefill_weights"] = PW

    def go(on, new):
        torch.cuda.synchronize()
        t = time.perf_counter()
        if on:
            ids, st = model.generate(batch, max_new_tokens=new, temperature=0.1, do_sample=False, prompt_lookup_num_tokens=k,
                                     max_matching_ngram_size=G, return_lookup_stats=True, **kw)
        else:
            ids, st = model.generate(batch, max_new_tokens=new, temperature=0.1, do_sample=False, **kw), None
        torch.cuda.synchronize()
        return time.perf_counter() - t, ids, st

    for on in (True, False):
        go(on, 2)                                          # warm-up (and the MXFP8 copies, if asked for)
    t1, tn, res = {True: [], False: []}, {True: [], False: []}, {}
    for _ in range(3):                                     # alternating
        for on in (True, False):
            t1[on].append(go(on, 1)[0])
            dt, ids, st = go(on, N)
            tn[on].append(dt)
            res[on] = (ids, st)
    a, b = min(t1[False]), min(tn[False])
    step = (b - a) / (N - 1) * 1e3
    print(f"B={B} S={S}{' decode_weights ' + DW if DW else ''} plain greedy: prefill+1 token {a * 1e3:.1f} ms; {step:.3f} ms/step = ms/token "
          f"({B / step * 1e3:.0f} tok/s)", flush=True)
    a, b = min(t1[True]), min(tn[True])
    ids, st = res[True]
    iters = int(st[:, 0].max()) - 1                        # verify iterations behind the prefill's step (sync_every = 16: a few more may be queued)
    per_it = (b - a) / max(iters, 1) * 1e3
    acc = float(st[:, 1].sum()) / max(B * iters, 1)
    tok = (N - 1) * B / (b - a)
    print(f"B={B} S={S}{' decode_weights ' + DW if DW else ''} lookup k={k} G={G}: prefill+1 token {a * 1e3:.1f} ms; {iters} verify iterations for {N - 1} "
          f"tokens per row; {per_it:.3f} ms/iteration = {per_it / step:.3f} x a plain step; {acc:.2f} accepted drafts per row and iteration "
          f"(random weights: the loops of this model, no estimate of a real one); {tok:.0f} tok/s ({tok / (B / step * 1e3):.2f} x plain); "
          f"ids equal plain: {torch.equal(ids, res[False][0])} (first column that differs, per row: "
          f"{[int((ids[r] != res[False][0][r]).int().argmax()) if bool((ids[r] != res[False][0][r]).any()) else None for r in range(B)]}); break-even at {per_it / step - 1:.2f} accepted drafts per iteration", flush=True)
    # the launches alone
    lc = model.model.config
    Hq, Hkv, D, L, Q = lc.num_attention_heads, lc.num_key_value_heads, lc.head_dim, 16, k + 1
    bf = torch.bfloat16
    Scap = S + N + Q
    q = torch.randn(B * Q, Hq, D, device="cuda", dtype=bf)
    kc = [torch.randn(B, Scap, Hkv, D, device="cuda", dtype=bf) for _ in range(2 * L)]
    base = torch.full((B,), S + N - 1, dtype=torch.int32, device="cuda")
    qkv = torch.randn(B * Q, (Hq + 2 * Hkv) * D, device="cuda", dtype=bf)

    def timed(name, fn, reps=6):
        for i in range(L):
            fn(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            for i in range(L):
                fn(i)
        e1.record()
        torch.cuda.synchronize()
        print(f"{name:74s} {e0.elapsed_time(e1) * 1e3 / (reps * L):7.1f} us/launch", flush=True)

    for _ in range(2):
        timed(f"attention, verify ({B} x {Q} positions over {Scap} keys, 2 launches)",
              lambda i: K.attn_decode_verify(q, kc[2 * i], kc[2 * i + 1], Q, None, base, D ** -0.5))
        timed(f"attention, plain step ({B} rows over {S + N} keys, 2 launches)",
              lambda i: K.attn_decode(q[:B], kc[2 * i][:, :S + N], kc[2 * i + 1][:, :S + N], None, D ** -0.5))
    timed(f"mm_kv_append_at ({B} x {Q} rows)", lambda i: K.lookup_append(qkv, B, Q, Hq, Hkv, D, base, kc[2 * i], kc[2 * i + 1]))
    st = K.LookupState(batch["input_ids"], batch["attention_mask"], k, G, N, model.config.eos_token_idx, S - 1)
    st.hlen += N - 1                                       # the history at the last step's length (the -1 fill matches itself: a full scan)
    tokq = torch.zeros(B * Q, dtype=torch.int64, device="cuda")
    timed(f"mm_lookup_draft ({B} rows, history {S + N - 1}, G = {G})", lambda i: K.lookup_draft(st))
    st.finished.fill_(1)                                   # the accept's launch without advancing the state
    timed(f"mm_lookup_accept ({B} rows)", lambda i: K.lookup_accept(st, tokq))


def compare_guidance(scale, kind):
    kw = {"decode_weights": DW} if DW else {}
    if PW:
        kw["prefill_weights"] = PW
    ids, mm = batch["input_ids"], batch["processed_multimodal_inputs"]
    none = {"batch_idx": {}, "token_range": {}, "stacked": {}}
    if kind == "text":                                     # the same rows without their image spans (every row loses as many positions)
        keep = torch.ones_like(ids, dtype=torch.bool)
        keep[mm["batch_idx"]["image"].long(), mm["token_range"]["image"].long()] = False
        nids = ids[keep].view(B, -1)
    else:
        nids = ids[:, -1:]
    Su = nids.shape[1]
    neg = dict(input_ids=nids, attention_mask=torch.ones(B, Su, dtype=torch.long, device="cuda"),
               position_ids=torch.arange(Su, device="cuda")[None, :].expand(B, Su).contiguous(), processed_multimodal_inputs=none)
    sides = {"plain": lambda new: model.generate(batch, max_new_tokens=new, temperature=0.1, do_sample=False, **kw),
             "unconditional alone": lambda new: model.generate(neg, max_new_tokens=new, temperature=0.1, do_sample=False, **kw),
             "guided": lambda new: model.generate(batch, max_new_tokens=new, temperature=0.1, do_sample=False, guidance_scale=scale,
                                                  negative_batch=neg if kind == "text" else None, **kw)}

    def go(name, new):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = sides[name](new)
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    for name in sides:
        go(name, 2)                                        # warm-up (and the MXFP8 copies, if asked for)
    t1, tn, shape = {k: [] for k in sides}, {k: [] for k in sides}, {}
    for _ in range(3):                                     # alternating
        for name in sides:
            t1[name].append(go(name, 1)[0])
            dt, out = go(name, N)
            tn[name].append(dt)
            shape[name] = tuple(out.shape)
    first, per = {}, {}
    for name in sides:
        a, b = min(t1[name]), min(tn[name])
        first[name], per[name] = a * 1e3, (b - a) / (N - 1) * 1e3
        print(f"B={B} S={S}{' decode_weights ' + DW if DW else ''} {name} ({Su if name == 'unconditional alone' else S} prompt positions): "
              f"prefill+1 token {first[name]:.1f} ms; decode {per[name]:.3f} ms/token (all runs "
              f"{', '.join(f'{(y - x) / (N - 1) * 1e3:.3f}' for x, y in zip(t1[name], tn[name]))}); ids {shape[name]}", flush=True)
    two = per["plain"] + per["unconditional alone"]
    print(f"guidance_scale={scale} negative={kind} (Su = {Su}): guided step {per['guided']:.3f} ms = {per['guided'] / per['plain']:.2f} x plain "
          f"({per['plain']:.3f}) = {per['guided'] / two:.2f} x `2 x plain` ({two:.3f}: a plain step of the prompts + one of the unconditional "
          f"prompts); prefill+1 token {first['guided']:.1f} ms against {first['plain']:.1f} plain, "
          f"{first['plain'] + first['unconditional alone']:.1f} two-pass", flush=True)


if GUIDE:
    compare_guidance(*GUIDE)
    sys.exit(0)
if LOOKUP:
    compare_lookup(*LOOKUP)
    sys.exit(0)
if PROC:
    compare_processors(PROC)
    sys.exit(0)
if NB > 1:
    compare_beams(NB)
    sys.exit(0)
if NS > 1:
    compare_samples(NS)
    sys.exit(0)
run(2)
if PW:
    first = {}
    for pw in (None, PW):
        run(1, pw)
        first[pw] = min(run(1, pw)[0] for _ in range(3))
    print(f"B={B} S={S}: first step (prefill + 1 token) bf16 {first[None] * 1e3:.1f} ms; prefill_weights {PW} {first[PW] * 1e3:.1f} ms "
          f"({first[None] / first[PW]:.2f}x)")
t1, _ = run(1)
tn, ids = run(N)
per_tok = (tn - t1) / (N - 1)
wbytes = sum(p.numel() for p in model.model.parameters()) * 2
if DW:          # what a decode step reads now: the packed copies, plus what stays bf16 (norm weights, biases; the embedding rows are a gather)
    w8 = model.model._decode_w8
    packed = [t[0] for lay in w8["layers"] for t in lay.values()] + ([w8["lm_head"][0]] if w8["lm_head"] else [])
    copied = sum(sum(p.numel() for p in ps) for ps in (
        [lay.self_attn._wqkv.params + [lay.self_attn.o_proj.weight] + lay.mlp._wgu.params + [lay.mlp.down_proj.weight] for lay in model.model.model.layers]
        + [[model.model.lm_head.weight]])) * 2
    wbytes = wbytes - copied + sum(t.numel() for t in packed)
lc = model.model.config
kv_row = 2 * lc.num_key_value_heads * (lc.head_dim + lc.head_dim // 32 if KV else lc.head_dim * 2)      # bytes of K and V per position and layer
kvbytes = B * S * kv_row * lc.num_hidden_layers
print(f"B={B} S={S}{' sample ' + str(SAMPLE) if SAMPLE else ''}{' decode_weights ' + DW if DW else ''}{' kv_cache ' + KV if KV else ''}{' prefill_weights ' + PW if PW else ''}: prefill+1 token {t1 * 1e3:.1f} ms; decode {per_tok * 1e3:.2f} ms/token ({B / per_tok:.0f} tok/s); "
      f"weight stream {wbytes / per_tok / 1e12:.2f} TB/s of 8 (floor {wbytes / 8e12 * 1e3:.2f} ms/token); KV {kvbytes / 1e9:.3f} GB/token ({kv_row} B per position and layer)  ids {tuple(ids.shape)}")
