"""mm_beam_step / mm_beam_finish through the library against tests/beam_ref.py (rules a-g of include/mm_hip.h in fp64; that file is
held to transformers' beam search in tests/test_beam_cpu.py).

A case loads a state into the device buffer (running scores, the token and ancestor tables that spell the running sequences, a
partly filled finished set, the open flag), runs ONE step twice, and compares everything the step writes.  A case that is not near
(beam_ref: no two neighbours of the sorted top 2n + 1 and no finished-set comparison closer than TAU) must match exactly in tokens,
parents, the finished set (sequences, lengths, arrival numbers), the new ancestor table and the flags; scores must be within the
bound; the two runs must agree bit for bit.  At most 10 % of the cases may be near.

The bound.  lp = fl(s + fl(x - lse)), lse = fl(m + logf(S)), S = sum of V terms expf(x - m) <= 1: with u = 2^-24, expf and logf
within 2 ulp, the sum taken as 16 sequential adds per thread, an 8-level tree, 4 waves and C = ceil(V / 4096) chunks (each rescaled by
one expf and one product), the relative error of S is at most (2 + 16 + 8 + 4 + C + 4) u and
  |lp - ref| <= u ((34 + C) + 2 |log S| + |lse| + |x - lse| + |lp|) =: bound(lp).
A normalised score lp / d adds the rounding of d and of the quotient: (bound(lp) + 2 u |lp|) / d.  TAU is twice the largest bound any
case here can reach (|x| <= 16, |s| <= 4, V <= 2^17: about 2.3e-5), in the style of kernel_check.check_bound: derived, never fitted."""
import math

import pytest
import torch

from multimeditron_amd import kernels as K
from tests import beam_ref as BR

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
XMAX, SMAX = 16.0, 4.0


def lp_bound(lp, x_minus_lse, lse, logS, V):
    C = -(-V // 4096)
    return U32 * ((34 + C) + 2 * abs(logS) + abs(lse) + abs(x_minus_lse) + abs(lp))


# the largest bound: |log S| <= log V, |lse| <= XMAX + log V, |x - lse| <= 2 XMAX + log V, |lp| <= SMAX + 2 XMAX + log V
_LV = math.log(1 << 17)
TAU = 2 * U32 * ((34 + 32) + 2 * _LV + (XMAX + _LV) + (2 * XMAX + _LV) + (SMAX + 2 * XMAX + _LV))
assert TAU < 1e-4


def case(V, n, B, step, T, es=False, lp=1.0, eos="inside", dtype=torch.bfloat16, pad=5, inf=False, fill="some"):
    return dict(V=V, n=n, B=B, step=step, T=T, es=es, lp=lp, eos=eos, dtype=dtype, pad=pad, inf=inf, fill=fill)


def case_id(c):
    return (f"V{c['V']}-n{c['n']}-B{c['B']}-i{c['step']}of{c['T']}-es{c['es']}-lp{c['lp']:g}-eos{c['eos']}-"
            f"{'bf16' if c['dtype'] == torch.bfloat16 else 'f32'}-pad{c['pad']}{'-inf' if c['inf'] else ''}-F{c['fill']}")


BF, F32 = torch.bfloat16, torch.float32
CASES = [
    # step 0 (one row per prompt), the middle, the last step; V = 2n, a chunk tail, 32 chunks; n = 1, 2, 5, 16; B = 1, 3
    case(2, 1, 1, 0, 4), case(2, 1, 3, 2, 4, eos="outside", fill="full"), case(4, 2, 3, 0, 3, es=True), case(4, 2, 1, 1, 3, es="never"),
    case(10, 5, 3, 1, 6, es=True, fill="full"), case(32, 16, 1, 0, 5), case(32, 16, 3, 3, 5, eos="outside", lp=0.0),
    case(32, 16, 1, 4, 5, es="never", fill="full"),                                           # the last step: every candidate stops
    case(1003, 1, 3, 0, 8, pad=21), case(1003, 2, 3, 3, 8, es=True, eos="inside", fill="full"), case(1003, 2, 1, 7, 8, lp=0.0),
    case(1003, 5, 3, 2, 8, es="never", eos="outside", inf=True), case(1003, 5, 1, 0, 8, dtype=F32, eos="absent"),
    case(1003, 16, 3, 5, 8, es=False, fill="full", dtype=F32, pad=3), case(1003, 16, 1, 7, 8, es=True, inf=True),
    case(1003, 5, 3, 4, 8, es=True, fill="none", eos="inside"), case(1003, 2, 3, 1, 8, es="never", lp=0.0, fill="full", eos="absent"),
    case(128258, 1, 1, 0, 4, pad=62), case(128258, 2, 3, 1, 4, es=True), case(128258, 5, 1, 2, 4, es="never", eos="outside", inf=True),
    case(128258, 16, 1, 0, 4, eos="inside"), case(128258, 16, 1, 2, 4, fill="full", lp=0.0, pad=6),
    case(128258, 5, 3, 3, 4, es=True, fill="full", dtype=F32, pad=2),
]


def test_the_cases_cover_what_the_issue_lists():
    assert {c["V"] for c in CASES} >= {1003, 128258} and any(c["V"] == 2 * c["n"] for c in CASES)
    assert {c["n"] for c in CASES} == {1, 2, 5, 16} and {c["B"] for c in CASES} == {1, 3}
    assert {c["es"] for c in CASES} == {False, True, "never"} and {c["lp"] for c in CASES} == {0.0, 1.0}
    assert {c["eos"] for c in CASES} >= {"inside", "outside"} and any(c["inf"] for c in CASES)
    assert any(c["step"] == 0 for c in CASES) and any(c["step"] + 1 == c["T"] for c in CASES) and all(c["pad"] > 0 for c in CASES)
    assert any(c["step"] > 0 and c["fill"] == "full" and c["B"] == 3 for c in CASES)                  # a closed prompt is stepped
    assert any(c["step"] > 0 and c["fill"] == "full" and c["es"] is True for c in CASES)              # a full set under early_stopping
    for V in (1003, 128258):
        assert {c["n"] for c in CASES if c["V"] == V} == {1, 2, 5, 16}


_built = {}


def build(c):
    """the inputs of a case (CPU) and what the reference makes of them; computed once per case and left unchanged"""
    key = case_id(c)
    if key in _built:
        return _built[key]
    V, n, B, i, T = c["V"], c["n"], c["B"], c["step"], c["T"]
    R = B * n
    g = torch.Generator().manual_seed(1000 + V % 997 + 31 * n + 7 * B + i)
    rows = B if i == 0 else R
    x = (3.0 * torch.randn(rows, V, generator=g)).clamp(-XMAX, XMAX).to(c["dtype"])
    if c["dtype"] == F32:
        x = x.to(BF).to(F32) + torch.randn(rows, V, generator=g) * 1e-3           # values bf16 cannot hold
    if c["inf"]:
        x[torch.rand(rows, V, generator=g) < 0.1] = -math.inf
        x[:, :2 * n] = x[:, :2 * n].nan_to_num(neginf=0.0)                       # at least 2n finite logits per row
    s = -SMAX * torch.rand(R, generator=g, dtype=torch.float64)
    s = s.float().double()                                                       # the fp32 values the device holds
    tok = torch.randint(0, V, (T, R), generator=g, dtype=torch.int32)
    base = torch.arange(R) // n * n
    anc = (base[None, :] + torch.randint(0, n, (T, R), generator=g)).to(torch.int32)
    prompts = []
    for b in range(B):
        p = BR.Prompt(n)
        if i > 0:
            p.s = [float(v) for v in s[b * n:(b + 1) * n]]
            p.seq = [[int(tok[t, anc[t, b * n + j]]) for t in range(i)] for j in range(n)]
            nf = {"none": 0, "some": (b + n // 2) % (n + 1), "full": n}[c["fill"]]
            for k in range(nf):
                ln = 1 + (k + b) % i
                p.F.append([float(torch.tensor(-3.0 * (k + 1 + b) / (n + 1) - 0.01 * k).float()), k, [int(t) for t in torch.randint(0, V, (ln,), generator=g)]])
            p.fcount = nf
            p.F.sort(key=lambda e: (-e[0], e[1]))
            p.open = not (c["fill"] == "full" and b == 1)                        # one closed prompt among the full ones
        prompts.append(p)
    # eos from the reference's own ranking of prompt 0: inside the top n, in ranks n .. 2n - 1, or a token no candidate has
    lp0 = BR.log_probs(x[:1 if i == 0 else n]) + (torch.zeros(1, 1, dtype=torch.float64) if i == 0 else s[:n, None])
    C0 = BR.top_candidates(lp0, 2 * n)
    if c["eos"] == "inside":
        eos = C0[n // 2][2]
    elif c["eos"] == "outside":
        eos = C0[n + (n - 1) // 2][2]
    else:
        eos = next(t for t in range(V) if t not in {cc[2] for cc in C0})
    before = [p.copy() for p in prompts]
    lp = BR.log_probs(x)
    per = 1 if i == 0 else n
    res = [BR.step(p, lp[b * per:(b + 1) * per], i, T, eos, c["lp"], c["es"], tau=TAU) for b, p in enumerate(prompts)]
    _built[key] = dict(x=x, s=s, tok=tok, anc=anc, before=before, after=prompts, res=res, eos=eos, near=any(r["near"] for r in res),
                       done=BR.done(prompts, i, T, c["es"]))
    return _built[key]


def load(c, d):
    """the device state and the logits (row stride V + pad, NaN in the padding)"""
    V, n, B, i, T = c["V"], c["n"], c["B"], c["step"], c["T"]
    st = K.BeamState(B, n, T, V, "cuda")
    st.buf.fill_(0x7F)                                                           # nothing needs clearing: junk everywhere
    logits = torch.full((d["x"].shape[0], V + c["pad"]), float("nan"), dtype=c["dtype"])
    logits[:, :V] = d["x"]
    if i > 0:
        st.score.copy_(d["s"].float())
        st.tok.copy_(d["tok"])
        st.anc[i & 1].copy_(d["anc"])
        for b, p in enumerate(d["before"]):
            st.open[b] = int(p.open)
            st.fcount[b] = p.fcount
            for k in range(n):
                e = p.F[k] if k < len(p.F) else None
                slot = b * n + (k * 3 + 1) % n if math.gcd(3, n) == 1 else b * n + k      # slots are not kept sorted
                st.flen[slot] = len(e[2]) if e else 0
                st.fscore[slot] = e[0] if e else -math.inf
                st.fseqno[slot] = e[1] if e else 0
                if e:
                    st.fseq[slot, :len(e[2])] = torch.tensor(e[2], dtype=torch.int32)
    return st, logits.cuda()[:, :V]


def snapshot(st):
    torch.cuda.synchronize()
    return {name: getattr(st, name).cpu().clone() for name, _ in K.BEAM_FIELDS} | {"next_ids": st.next_ids.cpu().clone()}


@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_beam_step_contract(c):
    V, n, B, i, T = c["V"], c["n"], c["B"], c["step"], c["T"]
    d = build(c)
    eos = d["eos"]
    st, logits = load(c, d)
    pre = snapshot(st)
    K.beam_step(logits, st, i, eos, c["lp"], c["es"])
    got = snapshot(st)
    # after "done" further steps leave every F unchanged: a closed prompt, and early_stopping=True with a full set (near or not)
    for b, p0 in enumerate(d["before"]):
        if i > 0 and (not p0.open or (c["es"] is True and len(p0.F) >= n)):
            for name in ("fscore", "flen", "fseqno", "fseq"):
                a, b_ = pre[name][b * n:(b + 1) * n], got[name][b * n:(b + 1) * n]
                assert torch.equal(a.view(torch.int32), b_.view(torch.int32)), (b, name)
            assert not bool(got["open"][b]) or p0.open
    ids, scores, lens = (t.cpu() for t in K.beam_finish(st, n, eos))
    st2, logits2 = load(c, d)
    K.beam_step(logits2, st2, i, eos, c["lp"], c["es"])
    again = snapshot(st2)
    written = ("score", "parent", "fscore", "flen", "fseqno", "open", "fcount", "done", "next_ids")
    for name in written:                                                          # two launches, equal bits
        a, b_ = got[name], again[name]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b_.view(torch.int32) if b_.dtype == torch.float32 else b_), name
    assert torch.equal(got["tok"][i], again["tok"][i]) and torch.equal(got["anc"][(i + 1) & 1][:i + 1], again["anc"][(i + 1) & 1][:i + 1])
    print(f"{case_id(c)}: near = {d['near']}, TAU = {TAU:.3g}")
    if d["near"]:
        return                                                                    # counted below; nothing exact is promised
    lse = torch.logsumexp(d["x"].double(), -1)
    for b, (p, r) in enumerate(zip(d["after"], d["res"])):
        rows = slice(b * n, (b + 1) * n)
        assert got["next_ids"][rows].tolist() == r["tok"] and got["tok"][i, rows].tolist() == r["tok"], (b, got["next_ids"][rows], r["tok"])
        assert got["parent"][rows].tolist() == r["parent"], (b, got["parent"][rows], r["parent"])
        for j in range(n):
            want, have = r["score"][j], float(got["score"][b * n + j])
            if want == -math.inf:
                assert have == -math.inf
                continue
            row = (b if i == 0 else b * n + r["parent"][j])
            xv = float(d["x"][row, r["tok"][j]])
            bound = lp_bound(want, xv - float(lse[row]), float(lse[row]), float(lse[row]) - float(d["x"][row].max()), V)
            assert abs(have - want) <= bound, (b, j, have, want, bound)
        # the finished set, in the contract's order
        slots = [k for k in range(n) if int(got["flen"][b * n + k]) > 0]
        F = sorted(((-float(got["fscore"][b * n + k]), int(got["fseqno"][b * n + k]), k) for k in slots))
        assert len(F) == len(p.F) == min(int(got["fcount"][b]), n) and int(got["fcount"][b]) == p.fcount
        for (ns_, seqno, k), e in zip(F, p.F):
            ln = int(got["flen"][b * n + k])
            assert seqno == e[1] and got["fseq"][b * n + k, :ln].tolist() == e[2], (b, k, seqno, e)
            if seqno < d["before"][b].fcount:
                assert -ns_ == e[0], (b, k, -ns_, e[0])                              # an entry that was there: untouched
            else:                                                                 # lp / d_i with d_i >= 1: bound(lp) <= TAU / 2
                assert abs(-ns_ - e[0]) <= TAU / 2 + 2 * U32 * abs(e[0]), (b, k, -ns_, e[0])
        assert bool(got["open"][b]) == p.open, b
        # the new ancestor table and, through it, the running sequences
        new = got["anc"][(i + 1) & 1]
        for j in range(n):
            assert int(new[i, b * n + j]) == b * n + j
            if r["score"][j] > -math.inf:
                assert new[:i, b * n + j].tolist() == d["anc"][:i, b * n + r["parent"][j]].tolist()
                assert [int(got["tok"][t, new[t, b * n + j]]) for t in range(i + 1)] == p.seq[j]
        # mm_beam_finish: the set in order, eos behind the end
        for k, e in enumerate(p.F):
            o = b * n + k
            assert int(lens[o]) == len(e[2]) and ids[o].tolist() == e[2] + [eos] * (T - len(e[2])) and float(scores[o]) == -F[k][0]
        for k in range(len(p.F), n):
            assert int(lens[b * n + k]) == 0 and ids[b * n + k].tolist() == [eos] * T and float(scores[b * n + k]) == -math.inf
    assert bool(got["done"][0]) == d["done"]


def test_at_most_a_tenth_of_the_cases_is_near():
    near = [case_id(c) for c in CASES if build(c)["near"]]
    print(f"near: {len(near)} of {len(CASES)}: {near}")
    assert len(near) <= len(CASES) // 10, near
