"""The four prompt-lookup launches through the C ABI (include/mm_hip.h): mm_lookup_draft and mm_lookup_accept exact against
tests/lookup_ref.py, mm_kv_append_at exact against an index copy into a sentinel-filled cache, and mm_attn_decode_verify held to
  (a) the bits of mm_attn_decode (two launches, attn_decode_mfma = 1, the same nsplit) run on one row per (sequence, position) under
      the equivalent mask,
  (b) independently, the per-element fp64 bound of attn_check.decode_reference for that kernel's path,
  (c) intact guards around out and the workspace, every slice's record written.
The shapes are the smallest at which the kernels can go wrong: partial and several column tiles (Q against 16 / G), a slice edge
inside a row's new positions, the last slots of the view, a history longer than one sweep of the workgroup."""
import random

import pytest
import torch

from tests import attn_check as AC
from tests import lookup_ref as LR
from tests.kernel_check import Guarded, check_bits, lib, ptr, rc, sentinel_fill, verify_guards, options
from tests.test_lookup_cpu import HAND

pytestmark = pytest.mark.gpu
I32 = dict(dtype=torch.int32, device="cuda")


# ---- mm_lookup_draft ----------------------------------------------------------------------------------------------------------------
def run_draft(hs, k, G, eos, count=None, finished=None, base=None, max_new=64, ld=None):
    rows = len(hs)
    ld = ld or max(len(h) for h in hs) + 3
    hist = torch.full((rows, ld), -1, dtype=torch.int32)
    for r, h in enumerate(hs):
        hist[r, :len(h)] = torch.tensor(h, dtype=torch.int32)
    count = count or [0] * rows
    finished = finished or [0] * rows
    base = base or [100 + 7 * r for r in range(rows)]
    d = lambda v: torch.tensor(v, **I32)
    ids = torch.full((rows, k + 1), -5, dtype=torch.int64, device="cuda")
    pos = torch.full((rows, k + 1), -5, dtype=torch.int64, device="cuda")
    nd = torch.full((rows,), -5, **I32)
    hist, hlen, count_d, fin_d, base_d = hist.cuda(), d([len(h) for h in hs]), d(count), d(finished), d(base)
    assert rc("mm_lookup_draft", ptr(hist), ld, ptr(hlen), ptr(count_d), ptr(fin_d), ptr(base_d), rows, k, G, max_new,
              -1 if eos is None else eos, ptr(ids), ptr(pos), ptr(nd)) == 0
    want = [LR.draft_row(h, k, G, eos, count[r], max_new, finished[r], base[r]) for r, h in enumerate(hs)]
    got = list(zip(ids.cpu().tolist(), pos.cpu().tolist(), nd.cpu().tolist()))
    for r in range(rows):
        assert got[r] == want[r], (r, hs[r], k, G, eos, got[r], want[r])
    return want


def test_draft_hand_and_random_cases_three_rows_at_a_time():
    by = {}
    for h, k, G, eos, want in HAND:
        by.setdefault((k, G, eos), []).append(h)
    rng = random.Random(11)
    for case in range(90):
        h = [rng.randrange(4) for _ in range(1 + (case * 7) % 40)]
        by.setdefault(((1, 3, 10)[case % 3], 1 + case % 4 % 3, (None, 3)[case % 2]), []).append(h)
    drafted = 0
    for (k, G, eos), hs in sorted(by.items(), key=str):
        while len(hs) % 3:
            hs.append(hs[0])
        for i in range(0, len(hs), 3):
            drafted += sum(w[2] > 0 for w in run_draft(hs[i:i + 3], k, G, eos))
    assert drafted > 30                                                   # the cases do draft


def test_draft_long_history_inactive_rows_clip_and_filler():
    h = list(range(100, 100 + 2560))                                      # all distinct ...
    h[2100], h[2101], h[-2], h[-1] = 7, 8, 7, 8                           # ... but for one 2-gram, whose only earlier occurrence lies past index 2048
    short = [1, 2, 7, 5, 6, 1, 2]
    w = run_draft([h, short, short], 3, 2, None, ld=2600)
    assert w[0] == ([8, 102 + 2100, 103 + 2100, 104 + 2100], [100, 101, 102, 103], 3)
    assert w[1] == ([2, 7, 5, 6], [107, 108, 109, 110], 3)
    # inactive rows (finished; count == max_new) draft nothing but still get ids[r, 0], the filler and pos; the clip to max_new - count - 1
    w = run_draft([short, short, short], 3, 2, None, count=[5, 64, 61], finished=[1, 0, 0], base=[9, 0, 2 ** 20])
    assert [x[2] for x in w] == [0, 0, 2] and w[0][0] == [2, 2, 2, 2] and w[2][0] == [2, 7, 5, 2] and w[2][1][3] == 2 ** 20 + 3
    w = run_draft([short, short, short], 10, 2, 5, count=[0, 62, 63])     # eos = 5 cuts [7, 5, 6, 1, 2] to [7]; one id of room; none
    assert [x[2] for x in w] == [1, 1, 0] and w[0][0] == [2, 7] + [2] * 9


# ---- mm_lookup_accept ---------------------------------------------------------------------------------------------------------------
def test_accept_chained_steps():
    rows, Q, max_new, eos, ld_hist = 3, 4, 10, 0, 24
    prompts = [[5, 6, 7], [8, 9], [4, 4, 4, 4, 4]]
    ref = [LR.Row(p, 40 + r, max_new, eos) for r, p in enumerate(prompts)]
    hist = torch.full((rows, ld_hist), -1, dtype=torch.int32)
    for r, p in enumerate(prompts):
        hist[r, :len(p)] = torch.tensor(p, dtype=torch.int32)
    d = lambda v: torch.tensor(v, **I32)
    st = dict(hist=hist.cuda(), hlen=d([len(p) for p in prompts]), count=d([0] * rows), fin=d([0] * rows), base=d([40, 41, 42]),
              stats=d([[0, 0]] * rows), done=d([7]), out=torch.full((rows, max_new + 2), eos, dtype=torch.int64, device="cuda"))
    # (ids, n_draft, tok) per row and step; step 0 is the prefill's token (Q = 1)
    X = [9, 9, 9, 9]
    steps = [
        (1, [([0], 0, [11]), ([0], 0, [21]), ([0], 0, [31])]),
        (4, [([11, 12, 13, 14], 3, [12, 13, 14, 15]),      # every draft accepted, and the bonus id
             ([21, 5, 5, 5], 3, [22, 5, 5, 5]),             # none
             ([31, 32, 33, 34], 3, [32, 33, 99, 34])]),     # a prefix
        (4, [([15, 16, 0, 18], 3, [16, 0, 18, 19]),         # eos inside an accepted run: the row ends there
             ([22, 22, 22, 22], 0, [23, 22, 22, 22]),       # no draft: the filler columns are no drafts
             ([99, 50, 51, 52], 3, [50, 51, 52, 53])]),     # count 4 -> 8
        (4, [(X, 3, X),                                     # a finished row: untouched
             ([23, 24, 25, 26], 3, [24, 25, 26, 27]),       # count 3 -> 7
             ([53, 54, 55, 56], 3, [54, 55, 56, 57])]),     # the cap mid-run: 8 -> 10, two of four
        (4, [(X, 3, X), ([27, 28, 29, 30], 3, [28, 29, 30, 31]), (X, 3, X)]),      # row 1: 7 -> 10; done
        (4, [(X, 3, X), (X, 3, X), (X, 3, X)]),             # a call after done
    ]

    def snapshot():
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in st.items()}

    for i, (q, rows_) in enumerate(steps):
        ids = torch.tensor([r[0] for r in rows_], dtype=torch.int64, device="cuda")
        nd = d([r[1] for r in rows_])
        tok = torch.tensor([r[2] for r in rows_], dtype=torch.int64, device="cuda")
        before = snapshot()
        assert rc("mm_lookup_accept", ptr(tok), ptr(ids) if q > 1 else None, ptr(nd) if q > 1 else None, rows, q, max_new, eos, ptr(st["out"]),
                  st["out"].stride(0), ptr(st["hist"]), ld_hist, ptr(st["hlen"]), ptr(st["count"]), ptr(st["fin"]), ptr(st["base"]),
                  ptr(st["stats"]), ptr(st["done"])) == 0
        after = snapshot()
        for r, (ids_r, nd_r, tok_r) in enumerate(rows_):
            was_active = ref[r].active
            ref[r].accept(tok_r, ids_r, nd_r)
            h = after["hist"][r].tolist()
            assert h[:len(ref[r].h)] == ref[r].h and set(h[len(ref[r].h):]) <= {-1}, (i, r, h, ref[r].h)
            assert after["out"][r].tolist() == ref[r].out + [eos] * (max_new + 2 - ref[r].count), (i, r)
            assert (int(after["hlen"][r]), int(after["count"][r]), int(after["fin"][r]), int(after["base"][r])) == \
                (len(ref[r].h), ref[r].count, int(ref[r].finished), ref[r].base), (i, r)
            assert after["stats"][r].tolist() == [ref[r].steps, ref[r].accepted], (i, r)
            if not was_active:                              # a row that is not active changes nothing
                for k in ("hist", "out", "hlen", "count", "fin", "base", "stats"):
                    assert torch.equal(before[k][r], after[k][r]), (i, r, k)
        assert int(after["done"]) == int(not any(x.active for x in ref)) == int(i >= 4), i
        if i == 5:                                          # after done no buffer changes
            for k in st:
                assert torch.equal(before[k].view(torch.uint8), after[k].view(torch.uint8)), k
    assert [x.count for x in ref] == [7, 10, 10] and ref[0].finished


# ---- mm_kv_append_at ----------------------------------------------------------------------------------------------------------------
def test_kv_append_at_is_an_index_copy():
    B, Q, Hq, Hkv, D, Smax = 2, 3, 4, 2, 128, 12
    W = (Hq + 2 * Hkv) * D
    g = torch.Generator().manual_seed(3)
    x = sentinel_fill(torch.empty(B * Q, W + 64, dtype=torch.bfloat16))
    x[:, :W] = torch.randn(B * Q, W, generator=g).to(torch.bfloat16)
    x = x.cuda()[:, :W]
    base = [3, 10]                                          # row 1: slots 10, 11 and 12 = Smax, which is skipped
    gk, gv = Guarded(B * Smax * Hkv * D, torch.bfloat16, "cuda"), Guarded(B * Smax * Hkv * D, torch.bfloat16, "cuda")
    shape, stride = (B, Smax, Hkv, D), (Smax * Hkv * D, Hkv * D, D, 1)
    kc, vc = gk.view(shape, stride), gv.view(shape, stride)
    want_k, want_v = kc.clone(), vc.clone()
    for b in range(B):
        for j in range(Q):
            if base[b] + j < Smax:
                want_k[b, base[b] + j] = x[b * Q + j, Hq * D:(Hq + Hkv) * D].view(Hkv, D)
                want_v[b, base[b] + j] = x[b * Q + j, (Hq + Hkv) * D:].view(Hkv, D)
    base_d = torch.tensor(base, **I32)
    assert rc("mm_kv_append_at", 0, ptr(x), x.stride(0), B, Q, Hq, Hkv, D, ptr(base_d), ptr(kc), ptr(vc), kc.stride(0),
              kc.stride(1), Smax) == 0
    torch.cuda.synchronize()
    check_bits("k cache", kc, want_k)                       # only the B Q - 1 target rows changed: the rest is still the sentinel
    check_bits("v cache", vc, want_v)
    verify_guards([("k cache", gk, False), ("v cache", gv, False)])
    assert int((kc.view(torch.int16) != 0x7FC1).any(dim=-1).any(dim=-1).sum()) == B * Q - 1


# ---- mm_attn_decode_verify ----------------------------------------------------------------------------------------------------------
D = 128


def VC(Hq, Hkv, Q, Scap, Sp, ns, mask, base):
    return dict(Hq=Hq, Hkv=Hkv, Q=Q, Scap=Scap, Sp=Sp, ns=ns, mask=mask, base=base)


VERIFY = [
    VC(2, 2, 16, 70, 9, 3, None, [54, 10]),                 # G 1, a full tile; Scap - Q; chunk 24: the edge 24 inside [10, 26)
    VC(8, 2, 5, 200, 64, 3, "leftpad", [195, 64]),          # G 4, two tiles (4 + 1); chunk 67: the edge 67 inside [64, 69)
    VC(4, 2, 4, 70, 9, 1, "leftpad", [66, 9]),              # G 2, half a tile, one slice
    VC(4, 2, 2, 200, 64, "lib", None, [198, 99]),           # the library's 4 slices of 50: the edge 100 inside [99, 101)
    VC(2, 2, 1, 70, 64, 3, "leftpad", [69, 63]),            # Q = 1: a plain decode step with its length on the device
    VC(8, 2, 16, 200, 9, "lib", "leftpad", [184, 40]),      # G 4, four tiles; 4 slices of 50: the edge 50 inside [40, 56)
    VC(8, 2, 5, 70, 9, 3, None, [65, 20]),                  # G 4 across a tile; the edge 24 inside [20, 25)
    VC(2, 2, 4, 200, 64, 1, None, [196, 70]),
    VC(4, 2, 5, 70, 64, 3, "leftpad", [65, 46]),            # G 2, one partial tile; a row still inside its masked prompt; the edge 48 inside [46, 51)
]


def vc_id(c):
    return f"h{c['Hq']}x{c['Hkv']}-q{c['Q']}-cap{c['Scap']}-sp{c['Sp']}-{c['mask'] or 'nomask'}-ns{c['ns']}"


def test_the_verify_cases_cover_what_the_kernel_distinguishes():
    assert {c["Hq"] // c["Hkv"] for c in VERIFY} == {1, 2, 4} and {c["Q"] for c in VERIFY} == {1, 2, 4, 5, 16}
    assert {c["Scap"] for c in VERIFY} == {70, 200} and {c["Sp"] for c in VERIFY} == {9, 64} and {c["ns"] for c in VERIFY} == {1, 3, "lib"}
    assert any(c["Q"] == 16 and c["Hq"] == c["Hkv"] for c in VERIFY) and any(c["Q"] == 5 and c["Hq"] == 4 * c["Hkv"] for c in VERIFY)
    assert all(c["base"][0] == c["Scap"] - c["Q"] for c in VERIFY)
    for c in VERIFY:
        if c["ns"] != 1:
            ns = c["ns"] if c["ns"] != "lib" else lib().mm_attn_decode_verify_splits(2, c["Q"], c["Hkv"], c["Scap"])
            chunk = -(-c["Scap"] // ns)
            assert any(c["base"][1] < e < c["base"][1] + c["Q"] for e in range(chunk, c["Scap"], chunk)) or c["Q"] == 1, vc_id(c)


def run_verify(c, base_given, base_eff):
    """-> (got, want, ref, guards): the kernel on base_given; mm_attn_decode per (b, j) row and the fp64 reference on base_eff."""
    B, Hq, Hkv, Q, Scap, Sp = 2, c["Hq"], c["Hkv"], c["Q"], c["Scap"], c["Sp"]
    ns = lib().mm_attn_decode_verify_splits(B, Q, Hkv, Scap) if c["ns"] == "lib" else c["ns"]
    pm = AC.decode_mask(c["mask"], B, Sp, ns)                              # [B, Sp] or None
    full = torch.ones(B, Scap, dtype=torch.long)
    if pm is not None:
        full[:, :Sp] = pm
    g = torch.Generator().manual_seed(5 + Scap + Q + Hq)
    q = torch.randn(B * Q, Hq, D, generator=g).to(torch.bfloat16)
    big = torch.where(full == 0, 1000.0, 1.0)[:, :, None, None]            # masked prompt keys are loud, as attn_check.decode_operands' are
    k = (torch.randn(B, Scap, Hkv, D, generator=g) * big).to(torch.bfloat16)
    v = (torch.randn(B, Scap, Hkv, D, generator=g) * big).to(torch.bfloat16)
    # the operands as generate passes them: q inside fused q|k|v rows, the cache a view of a longer buffer; from base + Q on the NaN sentinel
    row = sentinel_fill(torch.empty(B * Q, (Hq + 2 * Hkv) * D, dtype=torch.bfloat16))
    row[:, :Hq * D] = q.reshape(B * Q, Hq * D)
    kc = sentinel_fill(torch.empty(B, Scap + 11, Hkv, D, dtype=torch.bfloat16))
    vc = sentinel_fill(torch.empty(B, Scap + 11, Hkv, D, dtype=torch.bfloat16))
    for b in range(B):
        kc[b, :base_eff[b] + Q], vc[b, :base_eff[b] + Q] = k[b, :base_eff[b] + Q], v[b, :base_eff[b] + Q]
    row, kc, vc = row.cuda(), kc.cuda(), vc.cuda()
    qd, kd, vd = row[:, :Hq * D].view(B * Q, Hq, D), kc[:, :Scap], vc[:, :Scap]
    out, ws, guards = AC.decode_buffers(B * Q, Hq, D, ns, "cuda")
    pmd = pm.cuda() if pm is not None else None
    scale = D ** -0.5
    base_d = torch.tensor(base_given, **I32)
    assert rc("mm_attn_decode_verify", 0, ptr(qd), ptr(kd), ptr(vd), B, Q, Scap, Sp, Hq, Hkv, D, qd.stride(0), qd.stride(1), *AC._s3(kd),
              *AC._s3(vd), ptr(pmd), ptr(base_d), scale, ptr(out), ptr(ws), ns) == 0
    # one row per (b, j) over k / v[b, :Scap], finite everywhere, under [mask[b] | ones up to base + j | zeros after]
    t = torch.arange(Scap)
    mrows = torch.stack([full[b] * (t <= base_eff[b] + j) for b in range(B) for j in range(Q)]).contiguous()
    qm, km, vm = AC.decode_place(q, k.repeat_interleave(Q, dim=0), v.repeat_interleave(Q, dim=0))
    mm = mrows.cuda()
    with options(attn_decode_mfma=1):
        want, g2, _ = AC.run_decode(qm, km, vm, mm, scale, ns)
    torch.cuda.synchronize()
    verify_guards(guards + g2)
    return out, want, AC.decode_reference(qm, km, vm, mm, scale)


@pytest.mark.parametrize("c", VERIFY, ids=[vc_id(c) for c in VERIFY])
def test_verify_decode_contract(c):
    got, want, ref = run_verify(c, c["base"], c["base"])
    worst = AC.check_decode(got, ref, "bf16-decode-mfma")
    print(f"{vc_id(c)}: err / (u E) = {worst:.3f}, bits equal = {torch.equal(got.view(torch.int16), want.view(torch.int16))}")
    check_bits("verify == mm_attn_decode per (sequence, position) under the equivalent mask", got, want)


def test_verify_decode_clamps_base():
    """base outside [0, Scap - Q] is clamped, not followed: the result is the clamped base's, and nothing outside the view is read (the
    cache behind the clamped rows' positions holds NaN)."""
    c = VC(4, 2, 4, 70, 9, 3, "leftpad", None)
    got, want, ref = run_verify(c, [500, -7], [66, 0])
    AC.check_decode(got, ref, "bf16-decode-mfma")
    check_bits("clamped base", got, want)
    assert not bool(ref["rows"][4])                     # sequence 1, position 0 sees key 0 alone, which its left pad hides: exactly 0
