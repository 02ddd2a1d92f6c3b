"""generate(prompt_lookup_num_tokens=k) on the reference-generated d128 fixture (B = 2, row 1 left-padded; plain greedy decoding loops
on one id per row, so a lookup has something to find).

Wiring, exact: K.lookup_draft, K.lookup_accept, K.lookup_append and the selector K.argmax_softmax are wrapped with recording spies.
Every recorded draft must be tests/lookup_ref.py's of "visible prompt ids + ids emitted so far", every accept its accept of the
recorded selector output, and the returned ids, the stats and the history left on the device must follow from them.

Equality with plain greedy decoding: asserted with no exceptions, after a precondition on the PLAIN run alone -- its top-2 logit gap
exceeds TAU at every step of every row.  A verify step differs from a plain step in where the decode attention cuts its slices (and
possibly in the streaming GEMM's M); TAU is 4 x the largest per-element difference that very change makes to the plain run's
per-step logits, measured between the library's default attn_decode_wgs and attn_decode_wgs = 1 (profiles/r11_prompt_lookup.md)."""
import pytest
import torch

from multimeditron_amd import kernels as K
from oracle import ref_cpu as R
from tests import lookup_ref as LR
from tests.model_utils import build_from_golden

pytestmark = pytest.mark.gpu

NEW = 24
# The largest |logit difference| between the plain run under the library's default attn_decode_wgs (768) and under attn_decode_wgs = 1,
# over the steps up to which the ids agree.  On this file's batch ("left", bf16 weights) the two runs' logits are bit-equal (0.0); the
# figure kept is the largest seen over the fixture's three golden batches and twenty variants of them with shifted text ids, on the
# bf16 weights and on the MXFP8 copies: 2^-6, one bf16 ulp of a logit in [2, 4) (the fixture's logits reach 2.2).
TAU_MEASURED = 0.015625
TAU = 4 * TAU_MEASURED     # 0.0625; the "left" batch's smallest top-2 gap is 0.094


@pytest.fixture(scope="module")
def gold(golden_dir):
    return R.load_golden("tiny_clip_llama_d128", golden_dir)


@pytest.fixture(scope="module")
def model(gold, tmp_path_factory):
    meta, w, v = gold
    return build_from_golden(meta, w, tmp_path_factory.mktemp("lookup16"), "bfloat16")


@pytest.fixture(scope="module")
def batch(gold):
    b = R.golden_batch(gold[2], "left")
    assert b["input_ids"].shape[0] == 2 and int((b["attention_mask"][1] == 0).sum()) > 0 and bool(b["attention_mask"][0].all())
    return b


def plain_trace(m, batch, **kw):
    """plain greedy generate -> (ids, the fp32 copies of the logits the selector saw at every step)"""
    calls, real = [], K.argmax_softmax

    def spy(x, V, T):
        calls.append(x.float().clone())
        return real(x, V, T)

    K.argmax_softmax = spy
    try:
        ids = m.generate(batch, max_new_tokens=NEW, do_sample=False, **kw)
    finally:
        K.argmax_softmax = real
    return ids, calls


def min_gap(ids, calls, eos):
    """the smallest top-2 logit gap over every step of every row that had not finished before it"""
    worst = float("inf")
    alive = torch.ones(ids.shape[0], dtype=torch.bool)
    for i in range(ids.shape[1]):
        top = calls[i].topk(2, dim=-1).values.cpu()
        gap = (top[:, 0] - top[:, 1])[alive]
        worst = min(worst, float(gap.min())) if gap.numel() else worst
        alive &= ids[:, i] != eos
    return worst


@pytest.fixture(scope="module")
def plain(model, batch):
    """plain greedy decoding and the precondition of every equality below"""
    model.model.drop_decode_weights()
    ids, calls = plain_trace(model, batch)
    gap = min_gap(ids, calls, model.config.eos_token_idx)
    print(f"plain greedy: smallest top-2 logit gap {gap:.4f} against TAU = {TAU}")
    assert gap > TAU, (gap, TAU)
    return ids


def _visible(batch):
    ids, mask = batch["input_ids"], batch["attention_mask"]
    return [[int(t) for t in ids[b][mask[b] != 0]] for b in range(ids.shape[0])]


class Spies:
    """records every call of the three K.lookup_* wrappers and of the selector"""

    def __init__(self, monkeypatch):
        self.drafts, self.accepts, self.selected, self.appends = [], [], [], 0
        real_d, real_a, real_p, real_s = K.lookup_draft, K.lookup_accept, K.lookup_append, K.argmax_softmax

        def draft(st):
            rec = dict(st=st, hist=st.hist.clone(), hlen=st.hlen.clone())
            out = real_d(st)
            rec.update(ids=st.ids.clone(), pos=st.pos.clone(), nd=st.n_draft.clone())
            self.drafts.append(rec)
            return out

        def accept(st, tok, Q=None):
            self.accepts.append(dict(st=st, tok=tok.clone(), Q=st.Q if Q is None else Q, ids=st.ids.clone(), nd=st.n_draft.clone()))
            return real_a(st, tok, Q)

        def append(*a, **kw):
            self.appends += 1
            return real_p(*a, **kw)

        def select(x, V, T):
            out = real_s(x, V, T)
            self.selected.append(dict(out=out.clone(), rows=x.shape[0], T=T))
            return out

        monkeypatch.setattr(K, "lookup_draft", draft)
        monkeypatch.setattr(K, "lookup_accept", accept)
        monkeypatch.setattr(K, "lookup_append", append)
        monkeypatch.setattr(K, "argmax_softmax", select)


def replay(sp, batch, k, G, max_new, eos):
    """The recorded calls against tests/lookup_ref.py -> (the rows' reference state, rejected drafts per row, the columns of every
    row's output that were accepted drafts)."""
    vis = _visible(batch)
    B, Sp = batch["input_ids"].shape
    rows = [LR.Row(v, Sp - 1, max_new, eos) for v in vis]
    Q = k + 1
    assert len(sp.accepts) == len(sp.drafts) + 1 == len(sp.selected) and sp.accepts[0]["Q"] == 1
    assert all(a["st"] is sp.accepts[0]["st"] for a in sp.accepts) and all(d["st"] is sp.accepts[0]["st"] for d in sp.drafts)
    assert sp.selected[0]["rows"] == B and all(s["rows"] == B * Q for s in sp.selected[1:])
    tok0 = sp.accepts[0]["tok"].cpu().tolist()
    assert tok0 == sp.selected[0]["out"].cpu().tolist()
    for r in range(B):
        assert rows[r].accept([tok0[r]], [0], 0) == [tok0[r]] and rows[r].base == Sp         # the first generated token's position
    rejected, drafted = [0] * B, [[] for _ in range(B)]
    for i, (d, a) in enumerate(zip(sp.drafts, sp.accepts[1:])):
        hist, hlen = d["hist"].cpu(), d["hlen"].cpu().tolist()
        ids, pos, nd = d["ids"].cpu().tolist(), d["pos"].cpu().tolist(), d["nd"].cpu().tolist()
        tok = a["tok"].cpu().view(B, Q).tolist()
        assert a["Q"] == Q and a["tok"].cpu().tolist() == sp.selected[i + 1]["out"].cpu().tolist(), i
        assert a["ids"].cpu().tolist() == ids and a["nd"].cpu().tolist() == nd, i
        for r in range(B):
            assert hist[r, :hlen[r]].tolist() == rows[r].h, (i, r)                         # visible prompt ids + ids emitted so far
            assert (ids[r], pos[r], nd[r]) == rows[r].draft(k, G), (i, r)
            c0 = rows[r].count
            new = rows[r].accept(tok[r], ids[r], nd[r])
            drafted[r] += list(range(c0, c0 + len(new) - 1))
            if new and len(new) - 1 < nd[r] and not rows[r].finished and rows[r].count < max_new:
                rejected[r] += 1
    return rows, rejected, drafted


def expected_ids(rows, eos):
    n = max(r.count for r in rows)
    ids = torch.full((len(rows), n), eos, dtype=torch.int64)
    for i, r in enumerate(rows):
        ids[i, :r.count] = torch.tensor(r.out, dtype=torch.int64)
    done = (ids == eos).to(torch.int8).cummax(dim=1).values.bool().all(dim=0)
    return ids[:, : int(torch.nonzero(done)[0]) + 1] if bool(done.any()) else ids


def check_wiring(sp, got, stats, batch, k, G, eos):
    rows, rejected, _ = replay(sp, batch, k, G, NEW, eos)
    assert torch.equal(got, expected_ids(rows, eos)), (got.tolist(), [r.out for r in rows])
    assert stats.dtype == torch.int32 and not stats.is_cuda and stats.tolist() == [[r.steps, r.accepted] for r in rows]
    st = sp.accepts[0]["st"]
    hist, hlen = st.hist.cpu(), st.hlen.cpu().tolist()
    for r, row in enumerate(rows):
        assert hlen[r] == len(row.h) and hist[r, :hlen[r]].tolist() == row.h and bool((hist[r, hlen[r]:] == -1).all()), r
        assert int(st.base[r]) == row.base and int(st.count[r]) == row.count
    return rows, rejected


def test_wiring_and_that_the_run_speculates(model, batch, plain, monkeypatch):
    m = model
    eos = m.config.eos_token_idx
    sp = Spies(monkeypatch)
    ids, stats = m.generate(batch, max_new_tokens=NEW, do_sample=False, temperature=0.7, prompt_lookup_num_tokens=3, return_lookup_stats=True)
    assert all(s["T"] == 0.7 for s in sp.selected)                          # the selector plain greedy uses, at the caller's temperature
    n_layers = len(m.model.model.layers)
    assert sp.appends == n_layers * len(sp.drafts)
    rows, rejected = check_wiring(sp, ids, stats, batch, 3, 2, eos)
    print(f"stats {stats.tolist()}, rejected {rejected}, ids {ids.tolist()}")
    assert any(r.accepted >= 1 and r.steps < r.count for r in rows), stats.tolist()       # fewer verify steps than emitted tokens
    assert sum(rejected) >= 1, rejected


@pytest.mark.parametrize("k,G", [(3, None), (7, None), (1, None), (3, 3)])
def test_ids_equal_plain_greedy(model, batch, plain, monkeypatch, k, G):
    sp = Spies(monkeypatch)
    kw = {} if G is None else dict(max_matching_ngram_size=G)
    ids, stats = model.generate(batch, max_new_tokens=NEW, do_sample=False, prompt_lookup_num_tokens=k, return_lookup_stats=True, **kw)
    check_wiring(sp, ids, stats, batch, k, G or 2, model.config.eos_token_idx)
    assert torch.equal(ids, plain), (ids.tolist(), plain.tolist())
    assert ids.dtype == torch.int64 and not ids.is_cuda
    if k > 1:
        assert int(stats[:, 0].min()) < NEW                                  # it did speculate


@pytest.mark.parametrize("sync_every", [1, 16])
def test_sync_every_gives_the_same_ids_and_stats(model, batch, plain, sync_every):
    ids, stats = model.generate(batch, max_new_tokens=NEW, do_sample=False, prompt_lookup_num_tokens=3, return_lookup_stats=True,
                                sync_every=sync_every)
    ref, ref_stats = model.generate(batch, max_new_tokens=NEW, do_sample=False, prompt_lookup_num_tokens=3, return_lookup_stats=True,
                                    sync_every=5)
    assert torch.equal(ids, ref) and torch.equal(stats, ref_stats) and torch.equal(ids, plain)


def test_an_eos_inside_an_accepted_run_ends_that_row_only(model, batch, plain, monkeypatch):
    m = model
    eos0 = m.config.eos_token_idx
    sp = Spies(monkeypatch)
    m.generate(batch, max_new_tokens=NEW, do_sample=False, prompt_lookup_num_tokens=3)
    rows, _, drafted = replay(sp, batch, 3, 2, NEW, eos0)
    # an id that one row emitted as an ACCEPTED draft, before its last column, and the other row never emits
    pick = None
    for r in range(2):
        for c in drafted[r]:
            e = rows[r].out[c]
            if pick is None and e != eos0 and e not in rows[1 - r].out and rows[r].out.index(e) + 1 < rows[r].count:
                pick = (r, e)
    assert pick is not None, [x.out for x in rows]
    r, e = pick
    m.config.eos_token_idx = e
    try:
        del sp.drafts[:], sp.accepts[:], sp.selected[:]
        ids, stats = m.generate(batch, max_new_tokens=NEW, do_sample=False, prompt_lookup_num_tokens=3, return_lookup_stats=True, sync_every=4)
        check_wiring(sp, ids, stats, batch, 3, 2, e)
    finally:
        m.config.eos_token_idx = eos0
    first = rows[r].out.index(e)
    assert ids[r].tolist() == rows[r].out[:first + 1] + [e] * (ids.shape[1] - first - 1), (ids.tolist(), rows[r].out)       # ends there
    assert ids.shape[1] == NEW and ids[1 - r].tolist() == rows[1 - r].out                                                # goes on


def test_decode_weights_mxfp8_equals_plain_greedy_on_the_same_copies(model, gold):
    """On the MXFP8 copies the "left" batch's plain run comes as close as 0.047 (< TAU) to a second choice, so it cannot carry the
    precondition; the golden "right" batch with its text ids shifted by 6 (mod 120: the ids below the special ones) does (0.164)."""
    m = model
    batch = dict(R.golden_batch(gold[2], "right"))
    ids0 = torch.as_tensor(batch["input_ids"]).clone()
    batch["input_ids"] = torch.where(ids0 < 120, (ids0 + 6) % 120, ids0)
    try:
        ref, calls = plain_trace(m, batch, decode_weights="mxfp8")
        gap = min_gap(ref, calls, m.config.eos_token_idx)
        print(f"plain greedy on the MXFP8 copies: smallest top-2 logit gap {gap:.4f} against TAU = {TAU}")
        assert gap > TAU, (gap, TAU)
        ids, stats = m.generate(batch, max_new_tokens=NEW, do_sample=False, prompt_lookup_num_tokens=3, decode_weights="mxfp8",
                                return_lookup_stats=True)
    finally:
        m.model.drop_decode_weights()
    assert torch.equal(ids, ref), (ids.tolist(), ref.tolist())
    assert int(stats[:, 1].sum()) >= 1


def _refused(m, batch, match, **kw):
    """generate raises ValueError naming the argument before anything is encoded or decoded"""
    def boom(*a, **k):
        raise AssertionError("generate went on")
    m.model.forward = boom
    m.embed_modalities_with_text = boom
    kw.setdefault("do_sample", False)
    try:
        with pytest.raises(ValueError, match=match):
            m.generate(batch, max_new_tokens=2, **kw)
    finally:
        del m.model.forward
        del m.embed_modalities_with_text


def test_generate_refuses_what_is_out_of_scope(model, batch):
    m = model
    L = dict(prompt_lookup_num_tokens=3)
    _refused(m, batch, "do_sample", do_sample=True, **L)
    for name, val in (("top_k", 5), ("top_p", 0.9), ("min_p", 0.1), ("seed", 3), ("generator", torch.Generator())):
        _refused(m, batch, name, **{name: val}, **L)
    _refused(m, batch, "num_beams", num_beams=2, **L)
    _refused(m, batch, "num_return_sequences", num_return_sequences=2, **L)
    _refused(m, batch, "kv_cache", kv_cache="mxfp8", **L)
    for name, val in (("repetition_penalty", 1.2), ("no_repeat_ngram_size", 3), ("min_new_tokens", 2), ("suppress_tokens", [1])):
        _refused(m, batch, "logits processors", **{name: val}, **L)
    for bad in (0, -1, True, 2.0, "3"):
        _refused(m, batch, "prompt_lookup_num_tokens", prompt_lookup_num_tokens=bad)
    for bad in (0, -2, True, 1.5):
        _refused(m, batch, "max_matching_ngram_size", max_matching_ngram_size=bad, **L)
    _refused(m, batch, "at most 16", prompt_lookup_num_tokens=8)              # B (k + 1) = 18
    _refused(m, batch, "at most 16", prompt_lookup_num_tokens=15)
    _refused(m, batch, "need prompt_lookup_num_tokens", return_lookup_stats=True)
    _refused(m, batch, "need prompt_lookup_num_tokens", max_matching_ngram_size=2)
    # a model lookup_ok refuses
    llm = m.model
    assert llm.lookup_ok(2, 3) is None and "rows" in llm.lookup_ok(2, 8)
    old = llm.config.head_dim
    llm.config.head_dim = 64
    try:
        assert "head_dim" in llm.lookup_ok(2, 3)
        _refused(m, batch, "cannot be used", **L)
    finally:
        llm.config.head_dim = old
    assert "lookup_ok" in [v[1] for v in llm.OPTIONS.values()]


def test_off_is_off(model, batch, plain, monkeypatch):
    sp = Spies(monkeypatch)
    ids = model.generate(batch, max_new_tokens=NEW, do_sample=False, prompt_lookup_num_tokens=None, max_matching_ngram_size=None)
    assert torch.equal(ids, plain)
    assert sp.drafts == [] and sp.accepts == [] and sp.appends == 0 and len(sp.selected) >= plain.shape[1]
