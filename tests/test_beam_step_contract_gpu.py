"""mm_beam_step / mm_beam_finish through the library against tests/beam_ref.py (rules a-g of include/mm_hip.h in fp64; that file is
held to transformers' beam search in tests/test_beam_cpu.py).

A case loads a state into the device buffer (running scores, the token and ancestor tables that spell the running sequences, a
partly filled finished set, the open flag), runs ONE step twice, and compares everything the step writes.  A case that is not near
(beam_ref: no two neighbours of the sorted top 2n + 1 and no finished-set comparison closer than TAU) must match exactly in tokens,
parents, the finished set (sequences, lengths, arrival numbers), the new ancestor table and the flags; scores must be within the
bound; the two runs must agree bit for bit.  At most 10 % of the cases may be near.

The vocabularies reach the chunk edges of mm_beam.hip (4096 logits per workgroup): an exact multiple, and a last chunk shorter than
K = 2n that holds the row maximum, supplies winners and runs out (zero keys).  The logits take the 16-byte loads and the scalar ones
(a row stride or a base pointer off 16 bytes) in both dtypes; exact ties are planted across the chunk boundary and across two bit-equal
rows; a loaded ancestor table has entries outside its prompt's rows (the step clamps them: the reference reads the clamped table).
The state, the workspace, next_ids and mm_beam_finish's outputs sit in kernel_check.Guarded storages -- K.BeamState allocates them
exactly, so a write past an end would otherwise land in the allocator's slack; next_ids and the finish outputs must be fully written.
Chained steps on the kernel's own state: tests/test_beam_chain_contract_gpu.py.

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
from tests.kernel_check import Guarded, ptr, rc, sentinel_fill, verify_guards

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


def case(V, n, B, step, T, es=False, lp=1.0, eos="inside", dtype=torch.bfloat16, pad=5, inf=False, fill="some", plant=False, ties=None,
         off=0, oob=False):
    """plant: the row maximum at token 4096 and two of the top 2n at V - 1 and V - 2 (the short last chunk supplies winners and runs
    out).  ties: exact ties at ranks n-1 | n and 2n-1 | 2n, "row": equal logits of one row on both sides of the 4096 boundary (order
    by token); "twin": two rows of a prompt with equal scores and bit-equal logits besides (order by row).  off: the logits start
    `off` elements into their buffer (a base pointer that is not 16-byte aligned).  oob: a tenth of the loaded ancestor table lies
    outside its prompt's rows (the reference reads the clamped table)."""
    return dict(V=V, n=n, B=B, step=step, T=T, es=es, lp=lp, eos=eos, dtype=dtype, pad=pad, inf=inf, fill=fill, plant=plant, ties=ties,
                off=off, oob=oob)


def case_id(c):
    return (f"V{c['V']}-n{c['n']}-B{c['B']}-i{c['step']}of{c['T']}-es{c['es']}-lp{c['lp']:g}-eos{c['eos']}-"
            f"{'bf16' if c['dtype'] == torch.bfloat16 else 'f32'}-pad{c['pad']}{'-inf' if c['inf'] else ''}-F{c['fill']}"
            f"{'-plant' if c['plant'] else ''}{'-ties' + c['ties'] if c['ties'] else ''}{'-off%d' % c['off'] if c['off'] else ''}"
            f"{'-oob' if c['oob'] else ''}")


def vec(c):
    """whether mm_beam_step takes its 16-byte loads for this case's logits (base and row stride both 16-byte aligned)"""
    size = 2 if c["dtype"] == torch.bfloat16 else 4
    return (c["off"] * size) % 16 == 0 and ((c["V"] + c["pad"]) * size) % 16 == 0


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
# the chunk edge: V an exact multiple of 4096, a last chunk of 1 and of 2n - 1 < K entries (it runs out: beam_part_kernel writes zero
# keys, beam_merge_kernel skips them); both dtypes on the 16-byte loads, step 0 and a middle step
_EDGE = ((4096, 8), (4097, 7), (4096 + 2 * 16 - 1, 1), (8192, 8))
CASES += [case(V, 16, (1, 3)[(k + s) % 2], s, 6, es=(False, True, "never")[(k + s) % 3], eos=("inside", "outside")[(k + (s > 0)) % 2],
               fill=("some", "full")[k % 2], dtype=dt_, pad=pad, plant=V > 4096)
          for k, ((V, pad), dt_) in enumerate((e, d) for e in _EDGE for d in (BF, F32)) for s in (0, 3)]
CASES += [
    case(4097, 1, 3, 2, 5, pad=7, plant=True),
    # the scalar loads: a row stride that is no multiple of 16 bytes in bf16; a base pointer that is not 16-byte aligned in both dtypes
    case(1003, 5, 3, 2, 8, pad=4), case(128258, 16, 1, 1, 4, pad=1, fill="full"),
    case(1003, 2, 3, 1, 8, off=1), case(1003, 5, 1, 0, 8, dtype=F32, pad=1, off=1),
    case(4097, 16, 3, 0, 6, pad=7, off=1, plant=True), case(8192, 16, 1, 2, 6, dtype=F32, pad=8, off=1, plant=True, es=True),
    # planted exact ties
    case(8192, 16, 1, 0, 6, pad=8, ties="row"), case(8192, 16, 3, 0, 6, pad=8, ties="row", dtype=F32, es="never"),
    case(8192, 16, 3, 3, 6, pad=8, ties="twin"), case(8192, 16, 1, 2, 6, pad=8, ties="twin", dtype=F32, eos="outside", fill="full"),
    # the clamp of the table entries
    case(1003, 5, 3, 4, 8, oob=True), case(8192, 16, 1, 5, 6, pad=8, oob=True, dtype=F32, fill="full", plant=True),
]
OOB = (-1, None, None, 1 << 20, -(1 << 31))              # None: base - 1 and base + n of the entry's prompt


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
    # the chunk edges: an exact multiple of 4096 (one and two chunks), a last chunk of 1 and of 2n - 1 entries; both dtypes, step 0 and
    # a middle step, on the 16-byte loads; the short chunk holds the row maximum
    for V in (4096, 4097, 4096 + 2 * 16 - 1, 8192):
        cs = [c for c in CASES if c["V"] == V and c["n"] == 16 and vec(c) and not c["ties"] and not c["oob"]]
        assert {(c["dtype"], c["step"] == 0) for c in cs} == {(BF, True), (BF, False), (F32, True), (F32, False)}, V
        assert all(0 < c["step"] < c["T"] - 1 for c in cs if c["step"]) and all(c["plant"] == (V > 4096) for c in cs)
    assert any(c["V"] == 4097 and c["n"] == 1 and c["plant"] for c in CASES)
    assert any(0 < c["V"] % 4096 < 2 * c["n"] for c in CASES) and {c["B"] for c in CASES if c["V"] in (4097, 4127)} == {1, 3}
    # the scalar loads: bf16 rows whose stride is no multiple of 16 bytes at one chunk and at 32; a misaligned base in both dtypes,
    # with more than one chunk too
    assert {c["V"] for c in CASES if c["dtype"] == BF and not c["off"] and ((c["V"] + c["pad"]) * 2) % 16} >= {1003, 128258}
    assert {c["dtype"] for c in CASES if c["off"] and ((c["V"] + c["pad"]) * (2 if c["dtype"] == BF else 4)) % 16 == 0} == {BF, F32}
    assert any(c["off"] and c["V"] > 4096 for c in CASES) and any(not vec(c) and c["dtype"] == BF and c["V"] > 4096 for c in CASES)
    assert any(vec(c) for c in CASES if c["dtype"] == BF) and any(vec(c) for c in CASES if c["dtype"] == F32)
    # exact ties at V = 8192: inside one row (step 0) and between two rows (a middle step), in both dtypes
    assert {(c["ties"], c["dtype"]) for c in CASES if c["ties"]} == {("row", BF), ("row", F32), ("twin", BF), ("twin", F32)}
    assert all(c["V"] == 8192 and c["n"] == 16 and (c["step"] == 0) == (c["ties"] == "row") and c["step"] + 1 < c["T"] for c in CASES if c["ties"])
    # a loaded table with entries outside the prompt's rows, at a middle step and at the last one
    assert {c["step"] + 1 == c["T"] for c in CASES if c["oob"]} == {False, True} and all(c["step"] > 1 for c in CASES if c["oob"])


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
    if c["plant"]:
        x[:, V - 2], x[:, V - 1] = 13.0, 14.0
        x[:, 4096] = 15.5
    if c["ties"]:
        # levels 15.9375, 15.875, ... (bf16 holds them) above everything drawn; a level at two tokens is an exact tie inside a row
        x = x.clamp(max=8.0)
        twin = c["ties"] == "twin"
        # the levels held by two tokens.  One row: level k is rank k, so ranks n-1 | n and 2n-1 | 2n tie.  Twin rows give every level
        # twice (four times where two tokens hold it): 14 ranks, then ranks 14 .. 17 (n-1 | n: row A's second token | row B's first),
        # 12 ranks, then ranks 30 .. 33 (2n-1 | 2n); n = 16
        two = (7, 14) if twin else (n - 1, 2 * n - 2)
        pairs = ((4095, 4096), (100, 8000))                # both sides of the chunk boundary
        for b in range(B):
            rows_ = [b] if i == 0 else [b * n + 1, b * n + 2]
            for lv in range(two[1] + 1):
                toks = pairs[two.index(lv)] if lv in two else (200 + 257 * lv,)
                for r_ in rows_:
                    x[r_, list(toks)] = 15.9375 - 0.0625 * lv
            if twin:
                x[rows_[1]] = x[rows_[0]]
                s[b * n:(b + 1) * n] = s[b * n:(b + 1) * n].clamp(max=-1.0)
                s[rows_[0]] = s[rows_[1]] = -0.25
    tok = torch.randint(0, V, (T, R), generator=g, dtype=torch.int32)
    base = torch.arange(R) // n * n
    anc = (base[None, :] + torch.randint(0, n, (T, R), generator=g)).to(torch.int32)
    anc_raw = anc
    if c["oob"]:
        anc_raw = anc.clone()
        hit = torch.rand(T, R, generator=g) < 0.1
        kind = ((hit.view(-1).long().cumsum(0) - 1) % len(OOB)).view(T, R)      # the kinds in turn, from the first row read
        for k, v in enumerate(OOB):
            val = torch.full((T, R), v, dtype=torch.int64) if v is not None else (base - 1 if k == 1 else base + n)[None, :].expand(T, R)
            anc_raw = torch.where(hit & (kind == k), val.to(torch.int32), anc_raw)
        assert all(int((hit[:i] & (kind[:i] == k)).sum()) > 0 for k in range(len(OOB))), "an out-of-range kind is missing"
        anc = torch.minimum(torch.maximum(anc_raw, base[None, :].to(torch.int32)), (base + n - 1)[None, :].to(torch.int32))
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
    for r in res:
        ranked = r["cands"]
        if c["ties"]:                                                            # the planted ties sit where the case wants them
            assert ranked[n - 1][0] == ranked[n][0] and ranked[2 * n - 1][0] == ranked[2 * n][0] and not r["near"], case_id(c)
            assert {ranked[n - 1][2], ranked[n][2]} == {4095, 4096} and (ranked[n - 1][1] != ranked[n][1]) == (c["ties"] == "twin")
        if c["plant"] and not c["ties"]:                                         # the short chunk supplies the best candidate
            assert ranked[0][2] == 4096 and {V - 1, V - 2} <= {t for _, _, t in ranked[:2 * n]}, case_id(c)
    _built[key] = dict(x=x, s=s, tok=tok, anc=anc, anc_raw=anc_raw, before=before, after=prompts, res=res, eos=eos,
                       near=any(r["near"] for r in res), done=BR.done(prompts, i, T, c["es"]))
    return _built[key]


def _guarded(t):
    """a tensor of t's shape and dtype (contiguous, any 4- or 8-byte dtype, or bytes) inside a kernel_check.Guarded storage of fp32
    words, sentinel-filled: the allocator's slack is gone, a write past either end lands in a guard band"""
    nbytes = t.numel() * t.element_size()
    assert nbytes % 4 == 0
    g = Guarded(nbytes // 4, torch.float32, t.device)
    return g, g.view((nbytes // 4,), (1,)).view(t.dtype).view(t.shape)


def guard_state(st):
    """move a K.BeamState's buffers (state, workspace, next_ids) into guarded storages; the field views follow the state buffer"""
    guards = {}
    off = {name: getattr(st, name).data_ptr() - st.buf.data_ptr() for name, _ in K.BEAM_FIELDS}
    guards["state"], buf = _guarded(st.buf)
    for name, dtype in K.BEAM_FIELDS:
        old = getattr(st, name)
        setattr(st, name, buf[off[name]:off[name] + 4 * old.numel()].view(dtype).view(old.shape))
    st.buf = buf
    guards["ws"], st.ws = _guarded(st.ws)
    guards["next_ids"], st.next_ids = _guarded(st.next_ids)
    assert st.buf.data_ptr() % 16 == 0 and st.ws.data_ptr() % 16 == 0
    return guards


def verify_state(guards):
    torch.cuda.synchronize()
    verify_guards([("state", guards["state"]), ("ws", guards["ws"], False), ("next_ids", guards["next_ids"])])


def finish_guarded(st, nrs, eos):
    """mm_beam_finish through the raw ABI into guarded outputs -> (ids, scores, lens) on the CPU, guards verified, fully written"""
    rows = st.B * nrs
    gi, ids = _guarded(torch.empty((rows, st.T), dtype=torch.int64, device="cuda"))
    gs, scores = _guarded(torch.empty(rows, dtype=torch.float32, device="cuda"))
    gl, lens = _guarded(torch.empty(rows, dtype=torch.int32, device="cuda"))
    assert rc("mm_beam_finish", ptr(st.buf), st.buf.numel(), st.B, st.n, st.T, nrs, int(eos), ptr(ids), ptr(scores), ptr(lens)) == 0
    torch.cuda.synchronize()
    verify_guards([("finish ids", gi), ("finish scores", gs), ("finish lens", gl)])
    return ids.cpu(), scores.cpu(), lens.cpu()


def load(c, d):
    """the device state in guarded storages and the logits (row stride V + pad, NaN in the padding and before the first row)"""
    V, n, B, i, T = c["V"], c["n"], c["B"], c["step"], c["T"]
    st = K.BeamState(B, n, T, V, "cuda")
    guards = guard_state(st)
    st.buf.fill_(0x7F)                                                           # nothing needs clearing: junk everywhere
    rows, ld = d["x"].shape[0], V + c["pad"]
    flat = torch.full((c["off"] + rows * ld,), float("nan"), dtype=c["dtype"])
    logits = flat.as_strided((rows, V), (ld, 1), c["off"])
    logits.copy_(d["x"])
    if i > 0:
        st.score.copy_(d["s"].float())
        st.tok.copy_(d["tok"])
        st.anc[i & 1].copy_(d["anc_raw"])
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
    dev = flat.cuda().as_strided((rows, V), (ld, 1), c["off"])
    assert (dev.data_ptr() % 16 == 0) == (c["off"] == 0)
    return st, dev, guards


def snapshot(st):
    torch.cuda.synchronize()
    return {name: getattr(st, name).cpu().clone() for name, _ in K.BEAM_FIELDS} | {"next_ids": st.next_ids.cpu().clone()}


@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_beam_step_contract(c):
    V, n, B, i, T = c["V"], c["n"], c["B"], c["step"], c["T"]
    d = build(c)
    eos = d["eos"]
    st, logits, guards = load(c, d)
    pre = snapshot(st)
    sentinel_fill(st.next_ids.view(torch.float32))                                # the step must write every one
    K.beam_step(logits, st, i, eos, c["lp"], c["es"])
    verify_state(guards)
    got = snapshot(st)
    # after "done" further steps leave every F unchanged: a closed prompt, and early_stopping=True with a full set (near or not)
    for b, p0 in enumerate(d["before"]):
        if i > 0 and (not p0.open or (c["es"] is True and len(p0.F) >= n)):
            for name in ("fscore", "flen", "fseqno", "fseq"):
                a, b_ = pre[name][b * n:(b + 1) * n], got[name][b * n:(b + 1) * n]
                assert torch.equal(a.view(torch.int32), b_.view(torch.int32)), (b, name)
            assert not bool(got["open"][b]) or p0.open
    ids, scores, lens = finish_guarded(st, n, eos)
    one = finish_guarded(st, 1, eos)
    verify_state(guards)                                                          # mm_beam_finish only reads the state
    for a, b_ in zip(one, (ids, scores, lens)):
        assert torch.equal(a, b_[::n])
    st2, logits2, guards2 = load(c, d)
    K.beam_step(logits2, st2, i, eos, c["lp"], c["es"])
    verify_state(guards2)
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
