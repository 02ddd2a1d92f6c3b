"""generate(repetition_penalty=, no_repeat_ngram_size=, min_new_tokens=, suppress_tokens=) on the reference-generated d128 fixture
(B = 2, row 1 left-padded with 7 pad ids that are also the eos id; plain greedy decoding loops on one id per row).

Wiring, exact: K.logits_process is wrapped with a recording spy.  Every recorded call must satisfy tests/logits_ref.py bit for bit on
its recorded input with the history "visible prompt ids, then the ids emitted so far" (eos ids of finished rows included); the id a
row emits must be the selector's choice on the recorded output (K.argmax_softmax, or K.sample with the same seed and offset); the
history left on the device must be exactly that.  Properties: each is first shown to be VIOLATED without the argument (they fail on a
generate that swallows the arguments), then to hold with it.  Composition with num_return_sequences, the MXFP8 KV cache and MXFP8
decode weights; off is off; refusals before anything is encoded."""
import math

import numpy as np
import pytest
import torch

from multimeditron_amd import kernels as K
from oracle import ref_cpu as R
from tests import logits_ref as LR
from tests.model_utils import build_from_golden

pytestmark = pytest.mark.gpu

NEW = 12


@pytest.fixture(scope="module")
def gold(golden_dir):
    return R.load_golden("tiny_clip_llama_d128", golden_dir)


@pytest.fixture(scope="module")
def model(gold, tmp_path_factory):
    meta, w, v = gold
    return build_from_golden(meta, w, tmp_path_factory.mktemp("proc16"), "bfloat16")


@pytest.fixture(scope="module")
def batch(gold):
    b = R.golden_batch(gold[2], "left")
    assert b["input_ids"].shape[0] == 2 and int((b["attention_mask"][1] == 0).sum()) > 0 and bool(b["attention_mask"][0].all())
    return b


@pytest.fixture(scope="module")
def plain(model, batch):
    """greedy decoding without processors: it loops"""
    model.model.drop_decode_weights()
    return model.generate(batch, max_new_tokens=NEW, do_sample=False)


def _visible(batch, n=1):
    ids, mask = batch["input_ids"], batch["attention_mask"]
    return [[int(t) for t in ids[b][mask[b] != 0]] for b in range(ids.shape[0]) for _ in range(n)]


def _upto_eos(row, eos):
    row = [int(t) for t in row]
    return row[:row.index(eos) + 1] if eos in row else row


class Spy:
    """records every call of K.logits_process: input and output copies, step, last ids, the state"""

    def __init__(self, monkeypatch):
        self.calls = []
        real = K.logits_process

        def spy(logits2d, st, step, last_ids, eos):
            rec = dict(x=logits2d.clone(), step=step, last=last_ids.clone(), st=st, eos=eos, dtype=logits2d.dtype)
            out = real(logits2d, st, step, last_ids, eos)
            rec["out"] = out.clone()
            self.calls.append(rec)
            return out

        monkeypatch.setattr(K, "logits_process", spy)


def _check_wiring(spy, ids, batch, eos, V, kw, choose, n=1):
    """ids: what generate returned.  -> the emitted ids per row over all recorded calls"""
    calls = spy.calls
    vis = _visible(batch, n)
    rows = len(vis)
    assert [c["step"] for c in calls] == list(range(len(calls))) and len(calls) >= ids.shape[1] >= 1
    assert all(c["st"] is calls[0]["st"] for c in calls) and all(c["dtype"] == torch.bfloat16 and c["eos"] == eos for c in calls)
    emitted = torch.full((rows, len(calls)), eos, dtype=torch.int64)       # steps issued past the last returned one emit eos
    emitted[:, :ids.shape[1]] = ids
    finished = torch.zeros(rows, dtype=torch.bool)
    for i, c in enumerate(calls):
        assert c["x"].shape == (rows, V) and c["out"].shape == (rows, V) and c["out"].dtype == torch.float32
        hists = [vis[r] + emitted[r, :i].tolist() for r in range(rows)]
        want = LR.process(c["x"].float().cpu().numpy(), hists, i, **kw)
        assert LR.same_bits(c["out"].cpu().numpy(), want), f"step {i}: the kernel's output is not the reference's"
        if i > 0:
            assert torch.equal(c["last"].cpu(), emitted[:, i - 1]), f"step {i}: last_ids are not the ids of step {i - 1}"
        tok = choose(c["out"], i).cpu()
        for r in range(rows):
            assert int(emitted[r, i]) == (eos if finished[r] else int(tok[r])), (i, r)
        finished |= emitted[:, i] == eos
    st = calls[0]["st"]
    hist, plen = st.hist.cpu(), st.plen.cpu().tolist()
    for r in range(rows):
        assert plen[r] == len(vis[r])
        want = vis[r] + emitted[r, :len(calls) - 1].tolist()              # the id of the last call's step was not appended yet
        assert hist[r, :len(want)].tolist() == want, r
        assert bool((hist[r, len(want):] == -1).all()), r
    return emitted


def _run_with_an_eos_that_ends_one_row_early(m, batch, spy, kw, gen):
    """generate with config.eos_token_idx set to an id that one row emits at least two steps before the other row ends (the ids a run
    with the model's own eos emits from step min_new_tokens on are tried in turn) -> (eos, ids); the spy holds that run's calls"""
    eos0 = m.config.eos_token_idx
    base = m.generate(batch, max_new_tokens=NEW, **gen, **kw)
    cands = []
    for j in range(kw["min_new_tokens"], base.shape[1]):
        cands += [int(t) for t in base[:, j] if int(t) not in cands and int(t) != eos0]
    try:
        for e in cands[:10]:
            m.config.eos_token_idx = e
            del spy.calls[:]
            ids = m.generate(batch, max_new_tokens=NEW, sync_every=4, **gen, **kw)
            ends = sorted(len(_upto_eos(ids[r], e)) if e in ids[r].tolist() else NEW + 2 for r in range(ids.shape[0]))
            if ends[0] + 2 <= min(ends[-1], NEW):
                return e, ids
    finally:
        m.config.eos_token_idx = eos0
    raise AssertionError(f"no id of {cands} ends one row early: {base.tolist()}")


WIRING = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=4, suppress_tokens=[52, 122, 5, 5])


@pytest.mark.parametrize("path", ["greedy", "device-sampler"])
def test_every_step_goes_through_the_kernel_and_the_selector_reads_its_output(model, batch, plain, monkeypatch, path):
    m = model
    V = m._llm_cfg.vocab_size
    eos0 = m.config.eos_token_idx
    T = 0.7
    if path == "greedy":
        gen = dict(do_sample=False, temperature=T)
        choose = lambda out, i: K.argmax_softmax(out, V, T)
    else:
        gen = dict(do_sample=True, temperature=T, top_k=20, top_p=0.9, seed=11)
        choose = lambda out, i: K.sample(out, V, T, top_k=20, top_p=0.9, min_p=0.0, seed=11, offset=i)
    ref = dict(p=1.3, g=3, min_new_tokens=4, suppress=WIRING["suppress_tokens"])
    spy = Spy(monkeypatch)
    e, ids = _run_with_an_eos_that_ends_one_row_early(m, batch, spy, WIRING, gen)
    assert m.config.eos_token_idx == eos0
    emitted = _check_wiring(spy, ids, batch, e, V, dict(ref, eos=e), choose)
    # a row ended early and kept emitting eos into its history while the other went on
    ended = [len(_upto_eos(emitted[r], e)) for r in range(2)]
    assert min(ended) + 2 <= emitted.shape[1] and bool((emitted[ended.index(min(ended)), min(ended):] == e).all()), emitted.tolist()
    assert not bool((emitted[:, :4] == e).any()) and not any(t in (52, 122, 5) for t in emitted.flatten().tolist())


def test_no_repeat_ngram_size_ends_the_loop(model, batch, plain, monkeypatch):
    eos = model.config.eos_token_idx
    vis = _visible(batch)
    assert any(LR.repeats_ngram(vis[r] + _upto_eos(plain[r], eos), 3, len(vis[r])) for r in range(2)), plain.tolist()
    ids = model.generate(batch, max_new_tokens=NEW, do_sample=False, no_repeat_ngram_size=3)
    assert ids.shape[1] >= 3
    for r in range(2):
        assert not LR.repeats_ngram(vis[r] + _upto_eos(ids[r], eos), 3, len(vis[r])), ids.tolist()


def test_min_new_tokens_holds_eos_back(model, batch, plain):
    eos0, mn = model.config.eos_token_idx, 5
    e = int(plain[0, 0])
    model.config.eos_token_idx = e
    try:
        short = model.generate(batch, max_new_tokens=NEW, do_sample=False)
        assert bool((short[:, :mn] == e).any()), short.tolist()
        ids = model.generate(batch, max_new_tokens=NEW, do_sample=False, min_new_tokens=mn)
    finally:
        model.config.eos_token_idx = eos0
    assert ids.shape[1] >= mn and not bool((ids[:, :mn] == e).any()), ids.tolist()


def test_suppressed_ids_never_appear(model, batch, plain):
    sup = sorted(set(plain.flatten().tolist()) - {model.config.eos_token_idx})
    assert len(sup) >= 2
    ids = model.generate(batch, max_new_tokens=NEW, do_sample=False, suppress_tokens=sup + sup[:1])
    assert ids.shape[1] >= 1 and not set(ids.flatten().tolist()) & set(sup), (sup, ids.tolist())
    torch.manual_seed(3)
    drawn = model.generate(batch, max_new_tokens=NEW, temperature=1.0, suppress_tokens=sup)              # the torch.multinomial path
    assert not set(drawn.flatten().tolist()) & set(sup)


def test_repetition_penalty_changes_a_looping_output(model, batch, plain):
    assert all(len(set(plain[r, 1:].tolist())) == 1 for r in range(2)), plain.tolist()                      # the loop
    assert torch.equal(model.generate(batch, max_new_tokens=NEW, do_sample=False), plain)
    ids = model.generate(batch, max_new_tokens=NEW, do_sample=False, repetition_penalty=1.3)
    assert ids.shape != plain.shape or not torch.equal(ids, plain), ids.tolist()


@pytest.mark.parametrize("opt", ["num_return_sequences", "kv_cache", "decode_weights"])
def test_processors_compose_with_the_other_opt_ins(model, batch, plain, monkeypatch, opt):
    m = model
    eos = m.config.eos_token_idx
    n = 3 if opt == "num_return_sequences" else 1
    sup = sorted(set(plain.flatten().tolist()) - {eos})
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, suppress_tokens=sup)
    gen = {"num_return_sequences": dict(temperature=1.0, seed=7, num_return_sequences=3), "kv_cache": dict(do_sample=False, kv_cache="mxfp8"),
           "decode_weights": dict(do_sample=False, decode_weights="mxfp8")}[opt]
    spy = Spy(monkeypatch)
    try:
        ids = m.generate(batch, max_new_tokens=NEW, **gen, **kw)
    finally:
        m.model.drop_decode_weights()
    vis = _visible(batch, n)
    assert ids.shape[0] == 2 * n and ids.shape[1] >= 3 and len(spy.calls) >= ids.shape[1]
    for r in range(2 * n):
        assert not LR.repeats_ngram(vis[r] + _upto_eos(ids[r], eos), 3, len(vis[r])), (r, ids.tolist())
    assert not set(ids.flatten().tolist()) & set(sup)
    st = spy.calls[0]["st"]
    assert st.rows == 2 * n and st.plen.tolist() == [len(v_) for v_ in vis]
    hist, k = st.hist.cpu(), len(spy.calls) - 1
    emitted = torch.full((2 * n, len(spy.calls)), eos, dtype=torch.int64)
    emitted[:, :ids.shape[1]] = ids
    for r in range(2 * n):
        want = vis[r] + emitted[r, :k].tolist()
        assert hist[r, :len(want)].tolist() == want, r
    if n > 1:                                                   # the sample rows of a prompt went different ways: so did their histories
        assert any(not torch.equal(ids[b * n], ids[b * n + j]) for b in range(2) for j in range(1, n)), ids.tolist()


def test_off_is_off(model, batch, plain, monkeypatch):
    m = model
    spy = Spy(monkeypatch)
    off = dict(repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=None, suppress_tokens=None)
    neutral = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=[])
    sampled = m.generate(batch, max_new_tokens=NEW, temperature=0.8, top_k=20, seed=7)
    for kw in (off, neutral):
        assert torch.equal(m.generate(batch, max_new_tokens=NEW, do_sample=False, **kw), plain)
        assert torch.equal(m.generate(batch, max_new_tokens=NEW, temperature=0.8, top_k=20, seed=7, **kw), sampled)
    assert spy.calls == []
    m.generate(batch, max_new_tokens=2, do_sample=False, min_new_tokens=1)
    assert len(spy.calls) == 2 and spy.calls[0]["st"].hist is None          # no history buffer without the penalty or the ban


def _refused(m, batch, match, **kw):
    """generate raises ValueError naming the argument before anything is encoded or decoded"""
    def boom(*a, **k):
        raise AssertionError("generate went on")
    m.model.forward = boom
    m.embed_modalities_with_text = boom
    try:
        with pytest.raises(ValueError, match=match):
            m.generate(batch, max_new_tokens=2, do_sample=False, **kw)
    finally:
        del m.model.forward
        del m.embed_modalities_with_text


def test_generate_refuses_bad_values_and_beams(model, batch):
    V = model._llm_cfg.vocab_size
    for bad in (True, 0, 0.0, -1.3, math.nan, math.inf, "1.2"):
        _refused(model, batch, "repetition_penalty", repetition_penalty=bad)
    for bad in (True, -1, 2.5, "3"):
        _refused(model, batch, "no_repeat_ngram_size", no_repeat_ngram_size=bad)
    for bad in (True, -1, 1.5):
        _refused(model, batch, "min_new_tokens", min_new_tokens=bad)
    for bad in ([V], [-1], [True], [1.0], [3, V + 5], 5, "12"):
        _refused(model, batch, "suppress_tokens", suppress_tokens=bad)
    for name, val in (("repetition_penalty", 1.2), ("no_repeat_ngram_size", 3), ("min_new_tokens", 2), ("suppress_tokens", [1])):
        _refused(model, batch, f"num_beams=2 with {name}", num_beams=2, **{name: val})
    # the neutral values are no processors: beam search takes them
    ids = model.generate(batch, max_new_tokens=3, do_sample=False, num_beams=2, repetition_penalty=1.0, no_repeat_ngram_size=0,
                         min_new_tokens=0, suppress_tokens=[])
    assert ids.shape[0] == 2
