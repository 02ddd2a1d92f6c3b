"""The embedding checker has power (no GPU).  (a) A torch fp32 emulation of the three-kernel embedding gradient of
csrc/mm_embed.hip (sort, per-chunk runs with two scratch slots per chunk, merge) and of the movers passes tests/embed_check.py on
the cases tests/test_embed_contract_gpu.py runs.  (b) Each named mistake, applied to that emulation, is flagged on those same
cases -- by the exact-integer family, the bound, the poisoned scratch or a bit comparison."""
import contextlib

import pytest
import torch

from tests import embed_check as EC
from tests import test_embed_contract_gpu as GPU
from tests.embed_check import BF, F32, INVALID, R, VN
from tests.kernel_check import check_bits, sentinel_fill

DTYPES = [BF, F32]
ids = lambda d: EC.NAME[d] if isinstance(d, torch.dtype) else None


@pytest.fixture(autouse=True)
def _emulation_log():
    EC.PREFIX[0] = "emulation."
    yield
    EC.PREFIX[0] = ""


@contextlib.contextmanager
def as_mutant():
    """what a mutant measures goes under "mutant." in the ratio log, not among the emulation's own ratios"""
    old, EC.PREFIX[0] = EC.PREFIX[0], "mutant."
    try:
        yield
    finally:
        EC.PREFIX[0] = old


# ---- emulations (mut names a deliberate mistake) -------------------------------------------------------------------------------
def emu_sort(idt, smap, vocab, mut=None):
    T = idt.numel()
    k = EC.keys(idt, None if mut == "spliced_counted" else smap, vocab)
    if mut == "oob_into_row0":
        k = torch.where(k == INVALID, torch.zeros_like(k), k)
        if smap is not None:
            k = torch.where(smap >= 0, torch.full_like(k, INVALID), k)
    if mut == "unstable_sort":
        order = torch.tensor(sorted(range(T), key=lambda i: (int(k[i]), -i)), dtype=torch.int64)
    else:
        order = torch.tensor(sorted(range(T), key=lambda i: (int(k[i]), i)), dtype=torch.int64)
    n_order = EC.sizes(T, 1)[0]
    skey = torch.full((n_order,), INVALID, dtype=torch.int32)
    skey[:T] = k[order]
    return order.to(torch.int32), skey


def emu_demb(dE, order, skey, old, accumulate, mut=None):
    """the chunked reduction and the merge, chunk by chunk, with a NaN-poisoned scratch"""
    T, H = dE.shape
    dtype = dE.dtype
    nch = -(-T // R)
    part = sentinel_fill(torch.empty(nch, 2, H, dtype=F32))
    demb = old.clone()
    d32 = dE.float()
    live = H
    if mut == "ragged_slice_skipped" and H % (64 * VN[dtype]):
        live = H // (64 * VN[dtype]) * 64 * VN[dtype]

    def store(row, acc):
        out = acc + demb[row].float() if accumulate and mut != "accumulate_ignores_old" else acc
        demb[row, :live] = out.to(dtype)[:live]

    for c in range(nch):
        p0 = c * R
        ks = [int(x) for x in skey[p0:p0 + R]]
        if ks[0] == INVALID:
            continue
        kprev = int(skey[p0 - 1]) if c > 0 else -1
        knext = int(skey[p0 + R])
        run, at_start, acc = ks[0], True, torch.zeros(H)

        def flush(rk, at_start, at_end, acc):
            if rk == INVALID:
                return
            ts, te = at_start and kprev == rk, at_end and knext == rk
            if not ts and not te:
                store(rk, acc)
            else:
                part[c, 0 if ts else 1] = acc

        for i in range(R):
            if ks[i] != run:
                flush(run, at_start, False, acc)
                run, at_start, acc = ks[i], False, torch.zeros(H)
            if ks[i] != INVALID and not (mut == "chunk_last_dropped" and i == R - 1):
                acc = acc + d32[order[p0 + i]]
                if mut == "first_counted_twice" and i == 0 and kprev == ks[0]:
                    acc = acc + d32[order[p0]]
        flush(run, at_start, True, acc)
    for c in range(nch):
        p0 = c * R
        kl = int(skey[p0 + R - 1])
        if kl == INVALID or int(skey[p0 + R]) != kl:
            continue
        if int(skey[p0]) == kl and c > 0 and int(skey[p0 - 1]) == kl:
            continue
        acc = part[c, 1].clone()
        for cc in range(c + 1, nch):
            q0 = cc * R
            ends = not (int(skey[q0 + R - 1]) == kl and int(skey[q0 + R]) == kl)
            if mut == "merge_stops_early" and ends:
                break
            acc = acc + part[cc, 1 if mut == "merge_reads_slot1" else 0]
            if ends:
                break
        store(kl, acc)
    return demb


def case(name, seed=0):
    lengths, tail, mapper = GPU.DEMB_CASES[name]
    idt, vocab = EC.runs(lengths, tail, seed)
    return idt, vocab, (mapper(idt) if mapper else None)


def run_case(dtype, H, name, accumulate, exact, mut=None):
    idt, vocab, smap = case(name)
    T = idt.numel()
    order, skey = emu_sort(idt, smap, vocab, mut)
    dE, q = EC.exact_rows(T, H, dtype, "cpu", 1) if exact else (torch.randn(T, H, generator=torch.Generator().manual_seed(1)).to(dtype), None)
    old = EC.old_rows(vocab, H, dtype, "cpu")
    got = emu_demb(dE, order, skey, old, accumulate, mut)
    EC.check_demb(f"{name} H={H} acc={accumulate}", dE, idt, smap, vocab, old, accumulate, got, q)
    return order, skey


# ---- (a) the emulation passes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_embed_grad_emulation_passes(dtype):
    for name in GPU.DEMB_CASES:
        idt, vocab, smap = case(name)
        o_ref, k_ref = EC.sort_reference(idt, smap, vocab)
        for H in (GPU.WIDTHS[dtype][0], GPU.WIDTHS[dtype][2]):
            for accumulate in (0, 1):
                for exact in (False, True):
                    order, skey = run_case(dtype, H, name, accumulate, exact)
        assert bool((order == o_ref).all()) and bool((skey == k_ref).all()), name


def test_runs_place_the_edges():
    """the hand-placed cases hold what their names say"""
    def skey_of(name):
        idt, vocab, smap = case(name)
        return EC.sort_reference(idt, smap, vocab)[1]
    sk = skey_of("run ends on the edge")
    assert sk[30] != sk[31] != sk[32] and sk[63] == sk[32] and sk[64] == INVALID
    sk = skey_of("run starts on the last slot")
    assert sk[30] != sk[31] == sk[32] and sk[33] == INVALID
    sk = skey_of("chunk continues one run and starts another")
    assert sk[31] == sk[32] == sk[47] != sk[48] and sk[48] == sk[63] and sk[64] == INVALID
    sk = skey_of("invalid chunks behind 64 valid tokens")
    assert sk[63] != INVALID and bool((sk[64:] == INVALID).all()) and sk.numel() == 5 * R
    sk = skey_of("T % 32 == 0, the last run meets the padding")
    assert sk[10] == sk[63] != INVALID and sk.numel() == 3 * R
    assert bool((skey_of("every token out of range") == INVALID).all()) and bool((skey_of("every token under a splice") == INVALID).all())
    idt, vocab = EC.runs([3, 5], 2, 4)
    assert sorted(idt.tolist()) != idt.tolist() and torch.bincount(idt[(idt >= 0) & (idt < vocab)]).tolist() == [0, 3, 0, 5]


# ---- (b) the mutants are flagged -----------------------------------------------------------------------------------------------------
EMBED_MUTANTS = [  # (mutant, case, accumulate, widths: index into WIDTHS)
    ("chunk_last_dropped", "one id, two full chunks", 0, 0),
    ("chunk_last_dropped", "run ends on the edge", 0, 0),
    ("first_counted_twice", "one past the edge", 0, 0),
    ("first_counted_twice", "chunk continues one run and starts another", 1, 0),
    ("merge_stops_early", "one id, four chunks", 0, 0),
    ("merge_stops_early", "three runs over four chunks", 0, 0),
    ("merge_reads_slot1", "one id, two full chunks", 0, 0),
    ("merge_reads_slot1", "run starts on the last slot", 0, 0),
    ("spliced_counted", "every third token under a splice", 0, 0),
    ("spliced_counted", "every token under a splice", 0, 0),
    ("oob_into_row0", "invalid chunks behind 64 valid tokens", 0, 0),
    ("oob_into_row0", "every token out of range", 1, 0),
    ("ragged_slice_skipped", "three runs over four chunks", 0, 2),
    ("accumulate_ignores_old", "T = 1", 1, 0),
    ("accumulate_ignores_old", "one id, T = 200", 1, 0),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("mut,name,accumulate,wi", EMBED_MUTANTS, ids=[f"{m[0]}-{m[1]}" for m in EMBED_MUTANTS])
def test_embed_grad_mutant_is_flagged(dtype, mut, name, accumulate, wi):
    H = GPU.WIDTHS[dtype][wi]
    run_case(dtype, H, name, accumulate, True)
    with pytest.raises(AssertionError), as_mutant():
        run_case(dtype, H, name, accumulate, True, mut)            # the exact family: bit for bit


@pytest.mark.parametrize("mut,name", [("chunk_last_dropped", "one id, two full chunks"), ("first_counted_twice", "one past the edge"),
                                      ("merge_stops_early", "three runs over four chunks"), ("merge_reads_slot1", "one id, two full chunks")])
def test_embed_grad_mutant_is_flagged_by_the_bound_alone(mut, name):
    """fp32, random data: one token of a run of at most 64 is outside depth * sum|dE| * u32"""
    with pytest.raises(AssertionError), as_mutant():
        run_case(F32, 4, name, 0, False, mut)


def test_unstable_sort_is_flagged():
    for name in ("one id, two full chunks", "three runs over four chunks"):
        idt, vocab, smap = case(name)
        o_ref, k_ref = EC.sort_reference(idt, smap, vocab)
        order, skey = emu_sort(idt, smap, vocab, "unstable_sort")
        assert bool((skey == k_ref).all()) and not bool((order == o_ref).all())


# ---- movers and ViT glue -----------------------------------------------------------------------------------------------------------------
def test_patchify_swapped_grid_needs_a_non_square_image():
    def emu(pix, ps, kpad, dtype, swap):
        n, _, h, w = pix.shape
        g, gh = (h // ps, w // ps) if swap else (w // ps, h // ps)
        out = torch.zeros(n * g * gh, kpad, dtype=dtype)
        for i in range(n):
            for p in range(g * gh):
                py, px = p // g, p % g
                if (py + 1) * ps <= h and (px + 1) * ps <= w:
                    out[i * g * gh + p, :3 * ps * ps] = pix[i, :, py * ps:(py + 1) * ps, px * ps:(px + 1) * ps].reshape(-1).to(dtype)
        return out
    for h, w in [(28, 42), (42, 28), (30, 44)]:
        pix = torch.randn(3, 3, h, w)
        for dtype in DTYPES:
            for kpad in (588, 640):
                ref = EC.patchify_reference(pix, 14, kpad, dtype)
                check_bits("patchify", emu(pix, 14, kpad, dtype, False), ref)
                with pytest.raises(AssertionError), as_mutant():
                    check_bits("patchify", emu(pix, 14, kpad, dtype, True), ref)
    pix = torch.randn(3, 3, 28, 28)                                               # a square image cannot tell
    check_bits("patchify", emu(pix, 14, 588, F32, True), EC.patchify_reference(pix, 14, 588, F32))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_dpos_in_reverse_image_order_is_flagged(dtype):
    n, P, D = 3, 6, 72
    dx = EC.plant_order_triple(torch.randn(n, P + 1, D, generator=torch.Generator().manual_seed(9)).to(dtype))
    old_pos, old_cls = torch.randn(P + 1, D).to(dtype), torch.randn(D).to(dtype)
    for accumulate in (0, 1):
        _, dcls, dpos = EC.vit_embed_bwd_reference(dx, old_pos, old_cls, accumulate)
        s = (dx[0].float() + dx[1].float()) + dx[2].float()
        check_bits("dpos", (s + (old_pos.float() if accumulate else 0.0)).to(dtype), dpos)
        r = (dx[2].float() + dx[1].float()) + dx[0].float()
        if not accumulate or dtype == F32:                                       # (+ old moves a bf16 sum off the planted tie)
            with pytest.raises(AssertionError), as_mutant():
                check_bits("dpos reversed", (r + (old_pos.float() if accumulate else 0.0)).to(dtype), dpos)
    with pytest.raises(AssertionError), as_mutant():                                         # accumulate ignored
        check_bits("dcls", s[0].to(dtype), dcls)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_mover_mutants_are_flagged(dtype):
    x = torch.randn(5, 3, 72).to(dtype)
    wide = sentinel_fill(torch.empty(5, 3, 128, dtype=dtype))
    wide[..., :72] = x                                                          # the pad left unwritten
    ref = EC.head_pad_reference(x, 72, 128, False)
    wide_ok = wide.clone()
    wide_ok[..., 72:] = 0
    check_bits("head_pad", wide_ok, ref)
    with pytest.raises(AssertionError), as_mutant():
        check_bits("head_pad", wide, ref)
    src = torch.randn(6, 8).to(dtype)                                           # rows_select reading row n_src = 5 instead of a zero row
    idx = torch.tensor([0, 5, -1, 4, 7], dtype=torch.int32)
    ref = EC.rows_select_reference(src[:5], idx, 5)
    assert bool((ref[1] == 0).all()) and bool((ref[2] == 0).all()) and bool((ref[4] == 0).all())
    bad = ref.clone()
    bad[1] = src[5]
    with pytest.raises(AssertionError), as_mutant():
        check_bits("rows_select", bad, ref)


def test_splice_references():
    bi = torch.tensor([0, 0, 1, 0, 2, -1, 0])
    tr = torch.tensor([1, 1, 0, 1, 0, 1, 3])
    m = EC.build_map_reference(bi, tr, 4, 8)                                    # position 1 three times: index 3 wins; batch 2, -1: dropped
    assert m.tolist() == [-1, 3, -1, 6, 2, -1, -1, -1]
    dE = torch.arange(8.0)[:, None].expand(8, 4).contiguous()
    d = EC.dproj_reference(dE, bi, tr, 4, m)
    assert d[:, 0].tolist() == [0, 0, 4, 1, 0, 0, 3]
    emb, proj = torch.arange(5.0)[:, None].expand(5, 4), 100 + torch.arange(7.0)[:, None].expand(7, 4)
    out = EC.splice_fwd_reference(emb, torch.tensor([4, 4, 9, -1, 2, 3, 1, 0]), proj, m)
    assert out[:, 0].tolist() == [4, 103, 0, 106, 102, 3, 1, 0]
