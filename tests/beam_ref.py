"""Beam search selection restated in fp64: rules a-g of mm_beam_step (include/mm_hip.h), one step at a time on explicit state.

A step is *near* when its outcome could turn on fp32 rounding: two adjacent entries of the prompt's sorted top 2n + 1 log-probabilities
closer than tau without being an exact tie (equal logits of one row stay equal in any precision, their order is by token; and so
do equal values of two rows whose scores are equal and whose log-probability rows are bit-equal, their order is by row), or a comparison of the finished set (a new entry against the worst one, rule f's s_new[0] / d_L against the worst one) closer
than tau.  A caller that compares a kernel against this file holds every step that is not near to exact equality."""
import math

import torch

F64 = torch.float64


class Prompt:
    """one prompt's state: n running beams (score, sequence), the finished set as a list of [score, arrival, sequence] kept in the
    contract's order (higher score, then the earlier arrival), open, arrivals"""

    def __init__(self, n):
        self.n = n
        self.s = [0.0] * n
        self.seq = [[] for _ in range(n)]
        self.F = []
        self.open = True
        self.fcount = 0

    def copy(self):
        p = Prompt(self.n)
        p.s, p.seq, p.F = list(self.s), [list(q) for q in self.seq], [[e[0], e[1], list(e[2])] for e in self.F]
        p.open, p.fcount = self.open, self.fcount
        return p

    def worst(self):
        return min(e[0] for e in self.F)


def log_probs(x):
    """x [rows, V] (any float dtype) -> fp64 log-softmax rows"""
    x = x.to(F64)
    return x - torch.logsumexp(x, dim=-1, keepdim=True)


def top_candidates(lp, k):
    """lp [rows, V] fp64 -> the k largest as [(value, row, token)], descending, ties to the smaller flat index"""
    rows, V = lp.shape
    flat = lp.reshape(-1)
    k = min(k, flat.numel())
    thr = torch.topk(flat, k).values[-1]
    idx = torch.nonzero(flat >= thr).view(-1).tolist()
    cands = sorted(((-float(flat[i]), i) for i in idx))[:k]
    return [(-v, i // V, i % V) for v, i in cands]


def step(p: Prompt, lp_rows, i, T, eos, length_penalty=1.0, early_stopping=False, tau=0.0, select=top_candidates):
    """One step of one prompt.  lp_rows [1 (i = 0) or n, V]: fp64 log-probabilities of every row's continuations (log_probs of the
    logits).  Updates p; returns dict(tok, parent, score: the next running beams, entered: ranks that entered F, cands: the 2n
    candidates of rule b and the first one left out, near).  select: rule b itself (tests/beam_chain.py swaps in a deliberately wrong one)."""
    n = p.n
    rows = 1 if i == 0 else n
    assert lp_rows.shape[0] == rows
    s = torch.tensor([0.0] if i == 0 else p.s, dtype=F64)
    lp = s[:, None] + lp_rows.to(F64)                                       # a
    C = select(lp, 2 * n + 1)                                               # b (+ the first one left out)
    near = False
    for (v0, j0, t0), (v1, j1, t1) in zip(C, C[1:]):
        if v0 == -math.inf or v1 == -math.inf:
            continue
        same = j0 == j1 or (float(s[j0]) == float(s[j1]) and torch.equal(lp_rows[j0], lp_rows[j1]))
        if abs(v0 - v1) < tau and not (v0 == v1 and same):
            near = True
    ranked, C = C, C[:2 * n]
    last = i + 1 == T
    stop = [t == eos or last for _, _, t in C]                              # c
    run = [c for c, st in zip(C, stop) if not st][:n]                       # d
    full_before = len(p.F) >= n
    d_i = float(i + 1) ** length_penalty
    entered = []
    if p.open and not (early_stopping is True and full_before):             # e
        for rank in range(n):
            if not stop[rank]:
                continue
            v, j, t = C[rank]
            sv = v / d_i
            if len(p.F) >= n:
                w = p.worst()
                if abs(sv - w) < tau:
                    near = True
                if not sv > w:
                    continue
                p.F.pop()                                                   # the list is in order: the last one is the worst
            seq = ([] if i == 0 else list(p.seq[j])) + [t]
            p.F.append([sv, p.fcount, seq])
            p.fcount += 1
            p.F.sort(key=lambda e: (-e[0], e[1]))
            entered.append(rank)
    L = T if (isinstance(early_stopping, str) and early_stopping == "never" and length_penalty > 0) else i + 1
    if len(p.F) >= n:                                                       # f
        s0 = run[0][0] / float(L) ** length_penalty if run else -math.inf
        w = p.worst()
        if run and abs(s0 - w) < tau:
            near = True
        p.open = p.open and s0 > w
    old = p.seq
    new_s, new_seq, tok, parent = [], [], [], []
    for r in range(n):
        if r < len(run):
            v, j, t = run[r]
            new_s.append(v), new_seq.append(([] if i == 0 else list(old[j])) + [t]), tok.append(t), parent.append(j)
        else:                                                               # the last step: not used again
            new_s.append(-math.inf), new_seq.append(list(old[r])), tok.append(eos), parent.append(r)
    p.s, p.seq = new_s, new_seq
    return dict(tok=tok, parent=parent, score=new_s, entered=entered, cands=ranked, near=near)


def done(prompts, i, T, early_stopping):                                    # g
    return (not any(p.open for p in prompts)) or (early_stopping is True and all(len(p.F) >= p.n for p in prompts)) or i + 1 == T


def search(lp_fn, B, n, T, eos, length_penalty=1.0, early_stopping=False, nrs=1):
    """The whole call: lp_fn(i, seqs) -> fp64 log-probabilities [B * rows, V] for the running sequences seqs[b][j] (rows = 1 at
    i = 0, else n).  Returns (ids: list of token lists per returned row, scores, steps run)."""
    prompts = [Prompt(n) for _ in range(B)]
    steps = 0
    for i in range(T):
        rows = 1 if i == 0 else n
        lp = lp_fn(i, [p.seq for p in prompts])
        for b, p in enumerate(prompts):
            step(p, lp[b * rows:(b + 1) * rows], i, T, eos, length_penalty, early_stopping)
        steps = i + 1
        if done(prompts, i, T, early_stopping):
            break
    ids, scores = [], []
    for p in prompts:
        for e in p.F[:nrs]:
            ids.append(list(e[2]))
            scores.append(e[0])
    return ids, scores, steps
