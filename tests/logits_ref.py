"""The five rules of mm_logits_process (include/mm_hip.h) restated in numpy fp32, one row at a time, and transformers' four
processor classes chained in the same order.  A helper for tests/test_logits_process_*.py and tests/test_generate_processors_gpu.py,
not a test module."""
import numpy as np

LCHUNK = 4096                 # vocabulary entries per workgroup of the kernel (csrc/mm_logits.hip)


def process_row(x, h, step, p=1.0, g=0, min_new_tokens=0, eos=0, suppress=()):
    """x: the row's logits as fp32 [V]; h: the row's history (prompt ids, then emitted ids; L = plen + step entries) -> fp32 [V]"""
    x = np.array(x, dtype=np.float32)
    V = x.shape[0]
    h = [int(t) for t in h]
    L = len(h)
    p32 = np.float32(p)
    if p32 != np.float32(1.0):
        for v in sorted({t for t in h if 0 <= t < V}):          # once per id, from the unpenalised value
            with np.errstate(all="ignore"):
                x[v] = x[v] * p32 if x[v] < 0 else x[v] / p32
    if g > 0 and L + 1 >= g:
        tail = h[L - g + 1:]
        for i in range(0, L - g + 1):
            if h[i:i + g - 1] == tail and 0 <= h[i + g - 1] < V:
                x[h[i + g - 1]] = -np.inf
    if step < min_new_tokens:
        x[eos] = -np.inf
    for t in suppress:
        if 0 <= int(t) < V:
            x[int(t)] = -np.inf
    return x


def process(logits, hists, step, **kw):
    """rows of logits (fp32 [rows, V]) with one history per row -> fp32 [rows, V]"""
    return np.stack([process_row(logits[r], hists[r], step, **kw) for r in range(len(hists))])


def hf_process_row(x, h, step, p=1.0, g=0, min_new_tokens=0, eos=0, suppress=()):
    """the same row through transformers' classes as GenerationMixin chains them (a non-empty history of valid ids only)"""
    import torch
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor, SuppressTokensLogitsProcessor)
    ids = torch.tensor([list(h)], dtype=torch.long)
    s = torch.tensor(np.array(x, dtype=np.float32))[None, :].clone()
    if p != 1.0:
        s = RepetitionPenaltyLogitsProcessor(penalty=float(p))(ids, s)
    if g > 0:
        s = NoRepeatNGramLogitsProcessor(g)(ids, s)
    if min_new_tokens > 0:
        s = MinNewTokensLengthLogitsProcessor(len(h) - step, min_new_tokens, eos, device="cpu")(ids, s)
    if len(suppress):
        s = SuppressTokensLogitsProcessor([int(t) for t in suppress], device="cpu")(ids, s)
    return s[0].numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def repeats_ngram(seq, g, start=0):
    """whether a g-gram of seq that ENDS at index >= start (on a generated id, with start = the prompt's length) occurred before it;
    g-grams that lie inside the prompt may repeat each other (a run of placeholder ids does): no ban can undo those"""
    seen = set()
    for i in range(len(seq) - g + 1):
        t = tuple(seq[i:i + g])
        if t in seen and i + g - 1 >= start:
            return True
        seen.add(t)
    return False
