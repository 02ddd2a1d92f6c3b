"""Chained mm_beam_step runs on the state the steps themselves produce, against tests/beam_ref.py.

A *device* is anything that holds the state of include/mm_hip.h (mm_beam_state_layout's fields) and steps it: the library
(tests/test_beam_chain_contract_gpu.py) or the emulations below (tests/test_beam_chain_cpu.py, which shows that `run_chain` accepts a
right step and flags three wrong ones).  `run_chain` drives T steps without looking at `done` and checks after every one of them:

  the reference, teacher-forced.  The state before the step is decoded into beam_ref.Prompt objects (scores as the fp32 values held,
      sequences through tok[t, anc[i & 1][t, r]], F from the slots, open, fcount); beam_ref.step is applied with tau = tau_for(...);
      unless the step is near, everything the step wrote must equal it (scores within lp_bound).  A near step is counted and the run
      goes on from the device's own state, so one near step cannot derail the rest.
  the host mirror, near or not.  seqs[r] is kept on the host from `parent` and `next_ids` alone; the new table must spell exactly these
      sequences, lie inside its prompt's rows, and every finished entry that arrived must be one old mirrored sequence plus one token.
  F of a closed prompt, and of a full one under early_stopping=True, keeps its bits.

Logits are a pure function of (prompt, running sequence): a CPU generator seeded from a hash of the tokens, 3 randn(V) clamped to
+-16 in the case's dtype, the eos logit by the case's schedule -- what a real decoder gives, rows of equal sequence get equal logits.

tau.  TAU of tests/test_beam_step_contract_gpu.py is twice lp_bound at |s| <= SMAX = 4.  A chain's scores grow with its length (about
-1.5 a token here), and lp_bound carries the term u |lp|: one rounding of the sum s + (x - lse).  The near threshold of a step is
therefore TAU + 2 u max(0, max|s| - SMAX), the same expression at the scores the step actually reads: derived, never fitted."""
import hashlib
import math

import numpy as np
import torch

from tests import beam_ref as BR
from tests.test_beam_step_contract_gpu import SMAX, TAU, U32, XMAX, lp_bound

BF, F32 = torch.bfloat16, torch.float32
FIELDS = ("score", "parent", "tok", "anc", "fscore", "flen", "fseqno", "fseq", "open", "fcount", "done", "next_ids")
BCHUNK = 4096                                          # mm_beam.hip: vocabulary entries per workgroup


def tau_for(smax):
    return TAU + 2 * U32 * max(0.0, smax - SMAX)


def chain(name, n, B, V, T, es, lp, dtype, eos, sched, seed, expect):
    return dict(name=name, n=n, B=B, V=V, T=T, es=es, lp=lp, dtype=dtype, eos=eos, sched=sched, seed=seed, expect=expect)


# sched(i) -> None (the drawn logit stays), a bonus added to the drawn eos logit, or -inf.
# expect: what the CPU run (beam_ref on its own fp64 state, `predict`) gives for the seed: near (step, prompt) pairs and the
# coverage flags; tests/test_beam_chain_cpu.py asserts them, the GPU test asserts the same flags and the cap on what it saw.
CASES = [
    # steps 17..19: step * n > 256, a second trip of the ancestor copy
    chain("n16-T20", 16, 2, 1003, 20, False, 1.0, BF, 7, lambda i: 6.0 if i >= 6 else None, 1,
          dict(near=0, flags={"copy_trips": 2, "entered_on_eos": True, "closed_stepped": True})),
    # up to step * n = 595: three trips with a ragged tail; a full set replaces its worst entry (slot reuse)
    chain("n5-T120", 5, 3, 1003, 120, "never", 1.0, BF, 11, lambda i: 6.0 if i % 7 == 6 else None, 1,
          dict(near=0, flags={"copy_trips": 3, "ragged_tail": True, "replaced_worst": True, "entered_on_eos": True})),
    # eos never offered: F empty and the prompts open until the last step, where all n candidates enter with length 300
    chain("n2-T300", 2, 2, 64, 300, False, 1.0, BF, 3, lambda i: -math.inf, 1,
          dict(near=0, flags={"copy_trips": 3, "empty_until_last": True, "all_enter_last": True, "entered_len_over_256": True})),
    # entries longer than 256 arrive before the last step; the sets are then full under early_stopping=True and stay untouched
    chain("n3-T270", 3, 2, 64, 270, True, 0.0, BF, 5, lambda i: 8.0 if i >= 258 else -math.inf, 1,
          dict(near=1, flags={"copy_trips": 4, "entered_len_over_256_before_last": True, "full_es_stepped": True})),
    # one entry in the last chunk (token 4096 = eos): the short chunk supplies winners and then runs out
    chain("n16-V4097", 16, 1, 4097, 20, False, 1.0, F32, 4096, lambda i: 5.0 if i >= 3 else None, 1,
          dict(near=0, flags={"copy_trips": 2, "short_chunk_won": True, "entered_on_eos": True})),
]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def row_logits(c, b, seq, i):
    """the logits a decoder would give prompt b after the tokens seq (i = len(seq))"""
    h = hashlib.blake2b(np.asarray([c["seed"], b] + list(seq), dtype=np.int64).tobytes(), digest_size=8).digest()
    g = torch.Generator().manual_seed(int.from_bytes(h, "little") >> 1)
    x = (3.0 * torch.randn(c["V"], generator=g)).clamp(-XMAX, XMAX).to(c["dtype"])
    e = c["sched"](i)
    if e is not None:
        x[c["eos"]] = -math.inf if e == -math.inf else (x[c["eos"]].float() + e).clamp(-XMAX, XMAX).to(c["dtype"])
    return x


def step_logits(c, i, seqs):
    """[B (i = 0) or B n, V] for the running sequences seqs[b n + j]"""
    B, n = c["B"], c["n"]
    if i == 0:
        return torch.stack([row_logits(c, b, (), 0) for b in range(B)])
    return torch.stack([row_logits(c, r // n, seqs[r], i) for r in range(B * n)])


# ---- flags -------------------------------------------------------------------------------------------------------------------------
class Seen:
    """what a run met: near (step, prompt) pairs and the coverage flags of the issue"""

    def __init__(self, c):
        self.c, self.near, self.pairs, self.flags = c, [], 0, {}
        self.f_empty_open = True
        self.ratio = (0.0, -1)                        # the worst |score - reference| / lp_bound of a running beam, and its step

    def step(self, i, b, before, after, res):
        c = self.c
        n, T = c["n"], c["T"]
        self.pairs += 1
        if res["near"]:
            self.near.append((i, b))
        f = self.flags
        f["copy_trips"] = max(f.get("copy_trips", 0), -(-(i * n) // 256))
        if i * n > 256 and (i * n) % 256:
            f["ragged_tail"] = True
        cands = [res["cands"][k] for k in res["entered"]]
        if cands:
            if i + 1 < T:
                f["entered_on_eos"] = True
            if i >= 256:
                f["entered_len_over_256"] = True
                if i + 1 < T:
                    f["entered_len_over_256_before_last"] = True
            if len(before.F) + len(cands) > n:
                f["replaced_worst"] = True
            if c["V"] % BCHUNK and any(t >= c["V"] // BCHUNK * BCHUNK for _, _, t in cands) and c["V"] % BCHUNK < 2 * n:
                f["short_chunk_won"] = True
        if i > 0 and not before.open:
            f["closed_stepped"] = True
        if i > 0 and c["es"] is True and len(before.F) >= n:
            f["full_es_stepped"] = True
        if i + 1 < T and (after.F or not after.open):
            self.f_empty_open = False
        if i + 1 == T:
            if self.f_empty_open:
                f["empty_until_last"] = True
            if len(cands) == n and not before.F:
                f["all_enter_last"] = True

    def check(self, expect_flags):
        for k, v in expect_flags.items():
            got = self.flags.get(k, 0)
            assert (got >= v if isinstance(v, int) and not isinstance(v, bool) else got == v), (self.c["name"], k, got, v)
        assert 10 * len(self.near) <= self.pairs, (self.c["name"], len(self.near), self.pairs)


def predict(c):
    """the chain on the CPU alone: beam_ref evolving its own fp64 state -> Seen"""
    B, n, T = c["B"], c["n"], c["T"]
    prompts = [BR.Prompt(n) for _ in range(B)]
    seen = Seen(c)
    for i in range(T):
        x = step_logits(c, i, [s for p in prompts for s in p.seq])
        lp = BR.log_probs(x)
        per = 1 if i == 0 else n
        for b, p in enumerate(prompts):
            before = p.copy()
            smax = max([abs(v) for v in p.s if v > -math.inf] + [0.0])
            res = BR.step(p, lp[b * per:(b + 1) * per], i, T, c["eos"], c["lp"], c["es"], tau=tau_for(smax))
            seen.step(i, b, before, p, res)
    return seen


# ---- the state, decoded ------------------------------------------------------------------------------------------------------------
def decode(f, i, c):
    """the device state after i steps -> one beam_ref.Prompt per prompt (i = 0: the state no step has started)"""
    B, n = c["B"], c["n"]
    out = []
    if i > 0:
        table = f["anc"][i & 1][:i].long()
        seqs = f["tok"][:i].gather(1, table).t().tolist()                       # token t of running beam r is tok[t][anc[t][r]]
    for b in range(B):
        p = BR.Prompt(n)
        if i > 0:
            p.s = [float(v) for v in f["score"][b * n:(b + 1) * n]]
            p.seq = seqs[b * n:(b + 1) * n]
            for k in range(b * n, (b + 1) * n):
                ln = int(f["flen"][k])
                if ln > 0:
                    p.F.append([float(f["fscore"][k]), int(f["fseqno"][k]), f["fseq"][k, :ln].tolist()])
            p.F.sort(key=lambda e: (-e[0], e[1]))
            p.open, p.fcount = bool(f["open"][b]), int(f["fcount"][b])
        out.append(p)
    return out


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def written(f, i):
    """digest of everything step i wrote (the valid part of every finished sequence)"""
    h = hashlib.blake2b(digest_size=16)
    new = f["anc"][(i + 1) & 1]
    parts = [f[k] for k in ("score", "parent", "fscore", "flen", "fseqno", "open", "fcount", "done", "next_ids")] + [f["tok"][i], new[:i + 1]]
    for k in range(f["flen"].numel()):
        parts.append(f["fseq"][k, :max(int(f["flen"][k]), 0)])
    for t in parts:
        h.update(_bits(t).contiguous().numpy().tobytes())
    return h.digest()


def run_chain(dev, c, xs=None):
    """drive T steps of `dev` (reset(), step(x, i), fields(), finish(nrs)); every check of the module's docstring.  -> (Seen, the
    logits of every step, the digests of what every step wrote).  xs: replay these logits and only collect the digests."""
    B, n, T, V, eos = c["B"], c["n"], c["T"], c["V"], c["eos"]
    R = B * n
    dev.reset()
    replay = xs is not None
    xs = xs or []
    seen, digests = Seen(c), []
    mirror = [[] for _ in range(R)]
    f = dev.fields()
    state = decode(f, 0, c)
    base = torch.arange(R) // n * n
    for i in range(T):
        if replay:
            dev.step(xs[i], i)
            digests.append(written(dev.fields(), i))
            continue
        x = step_logits(c, i, mirror)
        xs.append(x)
        pre = f
        dev.step(x, i)
        f = dev.fields()
        digests.append(written(f, i))
        new = f["anc"][(i + 1) & 1]
        assert bool(((new[:i + 1] >= base) & (new[:i + 1] < base + n)).all()), f"step {i}: a table entry outside its prompt's rows"
        after = decode(f, i + 1, c)
        lp = BR.log_probs(x)
        lse = torch.logsumexp(x.double(), -1)
        per = 1 if i == 0 else n
        old_mirror = mirror
        mirror = [None] * R
        for b in range(B):
            rows = slice(b * n, (b + 1) * n)
            before, aft = state[b], after[b]
            # the host mirror: from parent and next_ids alone
            for j in range(n):
                par, t = int(f["parent"][b * n + j]), int(f["next_ids"][b * n + j])
                assert 0 <= par < n, (i, b, j, par)
                mirror[b * n + j] = ([] if i == 0 else list(old_mirror[b * n + par])) + [t]
                assert int(f["tok"][i, b * n + j]) == t and int(new[i, b * n + j]) == b * n + j, (i, b, j)
                if aft.s[j] > -math.inf:
                    assert aft.seq[j] == mirror[b * n + j], f"step {i}, row {b * n + j}: the table spells another sequence than parent / next_ids"
            arrived = [e for e in aft.F if e[1] >= before.fcount]
            olds = [[]] if i == 0 else [old_mirror[b * n + j] for j in range(n)]
            for e in arrived:
                assert len(e[2]) == i + 1 and e[2][:i] in olds and (e[2][i] == eos or i + 1 == T), \
                    f"step {i}, prompt {b}: finished entry {e[1]} is no running sequence plus a stopping token"
            # after "done": a closed prompt, and a full set under early_stopping=True, keep their bits
            if i > 0 and (not before.open or (c["es"] is True and len(before.F) >= n)):
                for name in ("fscore", "flen", "fseqno", "fseq"):
                    assert torch.equal(_bits(pre[name][rows]), _bits(f[name][rows])), (i, b, name)
                assert int(f["fcount"][b]) == before.fcount and (before.open or not aft.open), (i, b)
            # the reference on the state the device held
            ref = before.copy()
            smax = max([abs(v) for v in before.s if v > -math.inf] + [0.0])
            tau = tau_for(smax)
            res = BR.step(ref, lp[b * per:(b + 1) * per], i, T, eos, c["lp"], c["es"], tau=tau)
            seen.step(i, b, before, ref, res)
            if res["near"]:
                continue
            assert f["next_ids"][rows].tolist() == res["tok"] and f["parent"][rows].tolist() == res["parent"], \
                (i, b, f["next_ids"][rows].tolist(), res["tok"], f["parent"][rows].tolist(), res["parent"])
            for j in range(n):
                want, have = res["score"][j], aft.s[j]
                if want == -math.inf:
                    assert have == -math.inf, (i, b, j, have)
                    continue
                row = b if i == 0 else b * n + res["parent"][j]
                xv, ls = float(x[row, res["tok"][j]]), float(lse[row])
                bound = lp_bound(want, xv - ls, ls, ls - float(x[row].max()), V)
                seen.ratio = max(seen.ratio, (abs(have - want) / bound, i))
                assert abs(have - want) <= bound, (i, b, j, have, want, bound, abs(have - want) / bound)
                assert aft.seq[j] == ref.seq[j], (i, b, j)
                if i > 0:
                    assert new[:i, b * n + j].tolist() == pre["anc"][i & 1][:i, b * n + res["parent"][j]].tolist(), (i, b, j)
            assert len(aft.F) == len(ref.F) == min(ref.fcount, n) and aft.fcount == ref.fcount, (i, b, len(aft.F), len(ref.F), aft.fcount, ref.fcount)
            for e, w in zip(aft.F, ref.F):
                assert e[1] == w[1] and e[2] == w[2], (i, b, e, w)
                if e[1] < before.fcount:
                    assert e[0] == w[0], (i, b, e[0], w[0])                      # an entry that was there: untouched
                else:                                                            # lp / d_i, d_i >= 1: bound(lp) <= tau / 2
                    assert abs(e[0] - w[0]) <= tau / 2 + 2 * U32 * abs(w[0]), (i, b, e[0], w[0])
            assert aft.open == ref.open, (i, b)
        if not any(r for r in seen.near if r[0] == i):
            assert bool(f["done"][0]) == BR.done(after, i, T, c["es"]), i
        state = after
    if replay:
        return None, xs, digests
    # mm_beam_finish: the decoded finished sets in the contract's order, eos behind the end
    for nrs in (n, 1):
        ids, scores, lens = dev.finish(nrs)
        assert ids.shape == (B * nrs, T) and scores.shape == (B * nrs,) and lens.shape == (B * nrs,)
        for b, p in enumerate(state):
            for k in range(nrs):
                o = b * nrs + k
                if k < len(p.F):
                    e = p.F[k]
                    assert int(lens[o]) == len(e[2]) and ids[o].tolist() == e[2] + [eos] * (T - len(e[2])) and float(scores[o]) == e[0], (nrs, b, k)
                else:
                    assert int(lens[o]) == 0 and ids[o].tolist() == [eos] * T and float(scores[o]) == -math.inf, (nrs, b, k)
    return seen, xs, digests


# ---- an emulation of the step built from beam_ref ------------------------------------------------------------------------------------
def phantom_select(lp, k):
    """rule b of a kernel that takes the zero keys of a run-out chunk for candidates: the rounds past the end of a short last chunk
    hand out that chunk's last entry again"""
    rows, V = lp.shape
    tail, K = V % BCHUNK, k - 1
    if tail == 0 or tail >= K:
        return BR.top_candidates(lp, k)
    ext = torch.cat([lp, lp[:, V - 1:].expand(rows, K - tail)], 1)
    return [(v, j, min(t, V - 1)) for v, j, t in BR.top_candidates(ext, k)]


class Emulation:
    """The state layout in CPU tensors, stepped by beam_ref.step in fp64 with the scores stored as fp32.  fault:
      None          the contract
      "anc256"      the ancestor copy stops after 256 entries (no second trip of `for i = tid; i < step * n; i += 256`)
      "fseq255"     the finished-sequence copy stops at t = 255 (no second trip of `for t = tid; t <= step; t += 256`)
      "zero-keys"   the zero keys of a run-out chunk are taken as candidates"""

    def __init__(self, c, fault=None):
        self.c, self.fault = c, fault

    def reset(self):
        c = self.c
        B, n, T = c["B"], c["n"], c["T"]
        R = B * n
        J = 0x7F7F7F7F                                                             # nothing needs clearing: junk everywhere
        i32 = lambda *s: torch.full(s, J, dtype=torch.int32)
        self.f = dict(score=i32(R).view(torch.float32), parent=i32(R), tok=i32(T, R), anc=i32(2, T, R), fscore=i32(R).view(torch.float32),
                      flen=i32(R), fseqno=i32(R), fseq=i32(R, T), open=i32(B), fcount=i32(B), done=i32(1),
                      next_ids=torch.full((R,), J, dtype=torch.int64))

    def fields(self):
        return {k: v.clone() for k, v in self.f.items()}

    def step(self, x, i):
        c, f = self.c, self.f
        B, n, T = c["B"], c["n"], c["T"]
        prompts = decode(f, i, c)
        lp = BR.log_probs(x)
        per = 1 if i == 0 else n
        old, new = f["anc"][i & 1], f["anc"][(i + 1) & 1]
        select = phantom_select if self.fault == "zero-keys" else BR.top_candidates
        for b, p in enumerate(prompts):
            base = b * n
            if i == 0:
                f["flen"][base:base + n] = 0
                f["fscore"][base:base + n] = -math.inf
                f["fseqno"][base:base + n] = 0
            fcount0 = p.fcount
            res = BR.step(p, lp[b * per:(b + 1) * per], i, T, c["eos"], c["lp"], c["es"], select=select)
            kept = {e[1] for e in p.F}
            free = [k for k in range(base, base + n) if int(f["flen"][k]) == 0 or int(f["fseqno"][k]) not in kept]
            for e in sorted((e for e in p.F if e[1] >= fcount0), key=lambda e: e[1]):
                k = free.pop(0)
                f["fscore"][k], f["flen"][k], f["fseqno"][k] = e[0], len(e[2]), e[1]
                upto = min(len(e[2]), 256) if self.fault == "fseq255" else len(e[2])
                f["fseq"][k, :upto] = torch.tensor(e[2][:upto], dtype=torch.int32)
            for j in range(n):
                f["score"][base + j], f["parent"][base + j] = res["score"][j], res["parent"][j]
                f["tok"][i, base + j] = f["next_ids"][base + j] = res["tok"][j]
                new[i, base + j] = base + j
            for e in range(min(i * n, 256) if self.fault == "anc256" else i * n):
                t, r = e // n, e % n
                new[t, base + r] = old[t, base + res["parent"][r]]
            f["open"][b], f["fcount"][b] = int(p.open), p.fcount
        f["done"][0] = int(BR.done(prompts, i, T, c["es"]))

    def finish(self, nrs):
        c, f = self.c, self.f
        B, n, T, eos = c["B"], c["n"], c["T"], c["eos"]
        ids = torch.full((B * nrs, T), eos, dtype=torch.int64)
        scores = torch.full((B * nrs,), -math.inf, dtype=torch.float32)
        lens = torch.zeros(B * nrs, dtype=torch.int32)
        for b, p in enumerate(decode(f, T, c)):
            for k, e in enumerate(p.F[:nrs]):
                o = b * nrs + k
                ids[o, :len(e[2])] = torch.tensor(e[2])
                scores[o], lens[o] = e[0], len(e[2])
        return ids, scores, lens
