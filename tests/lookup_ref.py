"""The two rules of prompt-lookup decoding in plain Python (include/mm_hip.h: mm_lookup_draft, mm_lookup_accept).

draft: transformers' PromptLookupCandidateGenerator.get_candidates for one row (tests/test_lookup_cpu.py holds it to the installed
transformers), plus the clip to the room the row has left.  accept: the bookkeeping of one verify step for one row."""


def draft(h, k, G, eos=None, room=None):
    """The draft ids of a history h (list of ints): for g = min(G, L - 1) .. 1 the FIRST window i with h[i : i+g] == h[L-g :] and at least
    one id behind it wins, at the largest g that has one; the candidate is h[i+g : min(i+g+k, L)], cut before its first eos (an empty
    result is final: no other match is tried), then clipped to `room` ids."""
    h = [int(t) for t in h]
    L = len(h)
    for g in range(min(G, L - 1), 0, -1):
        tail = h[L - g:]
        for i in range(0, L - g):
            if h[i:i + g] == tail:
                start = i + g
                cand = h[start:min(start + k, L)]
                if eos is not None and eos in cand:
                    cand = cand[:cand.index(eos)]
                if room is not None:
                    cand = cand[:max(int(room), 0)]
                return cand
    return []


def draft_row(h, k, G, eos, count, max_new, finished, base):
    """mm_lookup_draft for one row -> (ids [k+1], pos [k+1], n_draft)."""
    active = (not finished) and count < max_new
    d = draft(h, k, G, eos, max_new - count - 1) if active else []
    last = int(h[-1])
    ids = [last] + d + [last] * (k - len(d))
    return ids, [base + j for j in range(k + 1)], len(d)


def accept(tok, ids, n_draft, count, max_new, eos, finished):
    """mm_lookup_accept for one row: tok [Q] the model's choice behind every verify position, ids [Q] the verify step's input ids (its
    draft at ids[1 : 1 + n_draft]).  -> (emitted ids, finished afterwards); an inactive row emits nothing."""
    if finished or count >= max_new:
        return [], bool(finished)
    a = 0
    while a < n_draft and int(ids[1 + a]) == int(tok[a]):
        a += 1
    out = []
    for j in range(a + 1):
        if count + len(out) >= max_new or finished:
            break
        out.append(int(tok[j]))
        if int(tok[j]) == eos:
            finished = True
    return out, bool(finished)


class Row:
    """The state mm_lookup_accept keeps for one row, advanced by the rule above."""

    def __init__(self, prompt, base, max_new, eos):
        self.h, self.base, self.max_new, self.eos = [int(t) for t in prompt], int(base), int(max_new), eos
        self.out, self.finished, self.steps, self.accepted = [], False, 0, 0

    @property
    def count(self):
        return len(self.out)

    @property
    def active(self):
        return (not self.finished) and self.count < self.max_new

    def draft(self, k, G):
        return draft_row(self.h, k, G, self.eos, self.count, self.max_new, self.finished, self.base)

    def accept(self, tok, ids, n_draft):
        if not self.active:
            return []
        new, self.finished = accept(tok, ids, n_draft, self.count, self.max_new, self.eos, self.finished)
        self.out += new
        self.h += new
        self.base += len(new)
        self.steps += 1
        self.accepted += len(new) - 1
        return new
