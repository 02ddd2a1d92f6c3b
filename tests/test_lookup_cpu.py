"""Prompt-lookup decoding without a device: the Python restatement of the draft rule against the installed transformers, the accept
rule on hand cases, the five new entry points (declared, exported, refusing before any launch) and the build's resource remarks of
the new kernels: no scratch."""
import ctypes
import os
import random

import pytest
import torch

from multimeditron_amd import _lib
from tests import lookup_ref as LR
from tests.test_no_spills_cpu import BUILD, _kernels

NEW = {"mm_lookup_draft": 15, "mm_kv_append_at": 15, "mm_attn_decode_verify_splits": 4, "mm_attn_decode_verify": 26, "mm_lookup_accept": 18}
UNSUPPORTED, ARG, ALIGN = -3, -1, -2
BF16, F32 = 0, 1


def hf_draft(h, k, G, eos):
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    gen = PromptLookupCandidateGenerator(eos_token_id=None if eos is None else torch.tensor([eos]), num_output_tokens=k,
                                         max_matching_ngram_size=G, max_length=10 ** 6)
    ids = torch.tensor([h], dtype=torch.long)
    cand, _ = gen.get_candidates(ids)
    return cand[0, len(h):].tolist()


HAND = [
    # history, k, G, eos, want
    ([1, 2, 3, 4], 3, 2, None, []),                                 # no match
    ([1, 2, 3, 9, 2], 3, 2, None, [3, 9, 2]),                       # a match only at g = 1
    ([1, 2, 7, 5, 1, 2, 8, 6, 1, 2], 2, 2, None, [7, 5]),           # two matches at g = 2: the first wins
    ([5, 6, 1, 2, 5, 6], 10, 2, None, [1, 2, 5, 6]),                # the continuation is cut by the end of the history
    ([4, 4, 4, 4], 3, 2, None, [4, 4]),                             # `aaaa`: windows overlap the tail
    ([1, 2, 0, 7, 1, 2], 3, 2, 0, []),                              # eos first: no draft, and no other match is tried
    ([1, 2, 7, 0, 8, 1, 2], 4, 2, 0, [7]),                          # eos in the middle
    ([3], 3, 2, None, []),                                          # L = 1
    ([3, 3], 3, 2, None, [3]),                                      # L = 2
    ([1, 2, 3, 1, 2, 9, 2, 3, 1, 2], 2, 3, None, [9, 2]),           # g = 3 (3 1 2 -> 9 2) beats the earlier g = 2 match (1 2 -> 3 1)
]


@pytest.mark.parametrize("h,k,G,eos,want", HAND)
def test_draft_hand_cases(h, k, G, eos, want):
    assert LR.draft(h, k, G, eos) == want
    assert hf_draft(h, k, G, eos) == want


def test_draft_equals_transformers_on_random_histories():
    rng = random.Random(7)
    n = 0
    for case in range(300):
        L = 1 + case % 40
        h = [rng.randrange(4) for _ in range(L)]
        for k in (1, 3, 10):
            for G in (1, 2, 3):
                for eos in (None, 3):
                    assert LR.draft(h, k, G, eos) == hf_draft(h, k, G, eos), (h, k, G, eos)
                    n += 1
    assert n == 300 * 18


def test_draft_row_fills_and_clips():
    h = [1, 2, 7, 5, 6, 1, 2]
    assert LR.draft_row(h, 3, 2, None, 0, 24, False, 40) == ([2, 7, 5, 6], [40, 41, 42, 43], 3)
    assert LR.draft_row(h, 5, 2, None, 0, 24, False, 40) == ([2, 7, 5, 6, 1, 2], [40, 41, 42, 43, 44, 45], 5)
    assert LR.draft_row(h, 3, 2, None, 21, 24, False, 9) == ([2, 7, 5, 2], [9, 10, 11, 12], 2)       # room = 24 - 21 - 1
    assert LR.draft_row(h, 3, 2, None, 23, 24, False, 9) == ([2, 2, 2, 2], [9, 10, 11, 12], 0)       # one id left: the verify row alone
    assert LR.draft_row(h, 3, 2, None, 24, 24, False, 9)[2] == 0 and LR.draft_row(h, 3, 2, None, 3, 24, True, 9)[2] == 0


def test_accept_rule():
    ids = [9, 5, 6, 7]
    assert LR.accept([5, 6, 7, 8], ids, 3, 0, 24, 0, False) == ([5, 6, 7, 8], False)          # every draft accepted + the bonus id
    assert LR.accept([4, 6, 7, 8], ids, 3, 0, 24, 0, False) == ([4], False)                   # none
    assert LR.accept([5, 6, 1, 8], ids, 3, 0, 24, 0, False) == ([5, 6, 1], False)             # a prefix, then the model's own id
    assert LR.accept([5, 6, 7, 8], ids, 1, 0, 24, 0, False) == ([5, 6], False)                # only n_draft columns are drafts
    assert LR.accept([5, 0, 7, 8], [9, 5, 0, 7], 3, 0, 24, 0, False) == ([5, 0], True)        # eos inside an accepted run ends the row
    assert LR.accept([5, 6, 7, 8], ids, 3, 22, 24, 0, False) == ([5, 6], False)               # the cap
    assert LR.accept([5, 6, 7, 8], ids, 3, 24, 24, 0, False) == ([], False) and LR.accept([5], ids, 0, 3, 24, 0, True) == ([], True)
    assert LR.accept([5], [9], 0, 0, 24, 0, False) == ([5], False)                            # Q = 1: the prefill's token
    r = LR.Row([1, 2, 3], 7, 4, 0)
    assert r.accept([5, 6], [3, 5], 1) == [5, 6] and (r.base, r.count, r.steps, r.accepted, r.h) == (9, 2, 1, 1, [1, 2, 3, 5, 6])
    assert r.accept([0, 1], [6, 0], 1) == [0] and r.finished and not r.active and r.accept([1, 1], [0, 1], 1) == [] and r.steps == 2


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_and_exported():
    protos = _lib.parse_header()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NEW.items():
        assert name in protos, f"include/mm_hip.h does not declare {name}"
        assert hasattr(L, name), f"libmmhip.so does not export {name}"
        assert len(protos[name][1]) == nargs, (name, len(protos[name][1]))
    assert L.mm_version() >= 102


def _buf():
    buf = ctypes.create_string_buffer(1 << 16)
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_draft_and_accept_refusals_come_before_any_launch():
    L = _lib.lib()
    keep, p = _buf()

    def draft(hist=p, ld=8, hlen=p, count=p, fin=p, base=p, rows=2, k=3, G=2, max_new=4, ids=p, pos=p, nd=p):
        return L.mm_lookup_draft(hist, ld, hlen, count, fin, base, rows, k, G, max_new, 0, ids, pos, nd, None)

    for name in ("hist", "hlen", "count", "fin", "base", "ids", "pos", "nd"):
        assert draft(**{name: None}) == ARG, name
    assert draft(rows=-1) == ARG and draft(rows=17) == ARG and draft(k=0) == ARG and draft(k=16) == ARG
    assert draft(G=0) == ARG and draft(max_new=0) == ARG and draft(ld=0) == ARG
    assert draft(rows=0) == 0

    def accept(tok=p, ids=p, nd=p, rows=2, Q=4, max_new=4, out=p, ld_out=4, hist=p, ld=8, hlen=p, count=p, fin=p, base=p, stats=p, done=p):
        return L.mm_lookup_accept(tok, ids, nd, rows, Q, max_new, 0, out, ld_out, hist, ld, hlen, count, fin, base, stats, done, None)

    for name in ("tok", "ids", "nd", "out", "hist", "hlen", "count", "fin", "base", "stats", "done"):
        assert accept(**{name: None}) == ARG, name
    assert accept(rows=-1) == ARG and accept(rows=17) == ARG and accept(Q=0) == ARG and accept(Q=17) == ARG
    assert accept(max_new=0) == ARG and accept(ld_out=3) == ARG and accept(ld=0) == ARG
    assert accept(rows=0) == 0 and accept(rows=0, Q=1, ids=None, nd=None) == 0         # Q = 1 takes no drafts


def test_append_refusals_come_before_any_launch():
    L = _lib.lib()
    keep, p = _buf()
    W = 4 * 128                                    # a fused q|k|v row of (2 + 1 + 1) heads

    def app(dtype=BF16, x=p, ld=W, B=2, Q=3, Hq=2, Hkv=1, D=128, base=p, kc=p, vc=p, sb=40 * 128, ss=128, Smax=40):
        return L.mm_kv_append_at(dtype, x, ld, B, Q, Hq, Hkv, D, base, kc, vc, sb, ss, Smax, None)

    for name in ("x", "base", "kc", "vc"):
        assert app(**{name: None}) == ARG, name
    assert app(B=-1) == ARG and app(Q=0) == ARG and app(Q=17) == ARG and app(Hq=0) == ARG and app(Hkv=0) == ARG and app(Smax=0) == ARG
    assert app(ld=W - 8) == ARG
    assert app(dtype=F32) == UNSUPPORTED and app(D=4, ld=W) == UNSUPPORTED
    assert app(ss=64) == ARG and app(sb=39 * 128) == ARG                                 # slots or sequences that would overlap
    assert app(ld=W + 4) == ALIGN and app(sb=40 * 128 + 4) == ALIGN and app(ss=132, sb=40 * 136) == ALIGN
    for name in ("x", "kc", "vc"):
        assert app(**{name: p + 8}) == ALIGN, name
    assert app(B=0) == 0


def test_verify_attention_refusals_come_before_any_launch():
    L = _lib.lib()
    keep, p = _buf()
    W = 4 * 128
    STRIDES = ("qsb", "qsh", "ksb", "kss", "ksh", "vsb", "vss", "vsh")

    def attn(dtype=BF16, q=p, k=p, v=p, B=2, Q=3, Scap=20, Sp=5, Hq=2, Hkv=1, D=128, mask=None, base=p, out=p, ws=p, ns=1, **st):
        s = dict(qsb=W, qsh=128, ksb=40 * 128, kss=128, ksh=128, vsb=40 * 128, vss=128, vsh=128)
        assert set(st) <= set(s)
        s.update(st)
        return L.mm_attn_decode_verify(dtype, q, k, v, B, Q, Scap, Sp, Hq, Hkv, D, *(s[n] for n in STRIDES), mask, base,
                                       ctypes.c_float(0.1), out, ws, ns, None)

    assert attn(D=64) == UNSUPPORTED and attn(dtype=F32) == UNSUPPORTED
    assert attn(Hq=8, Hkv=1) == UNSUPPORTED and attn(Hq=7, Hkv=1) == UNSUPPORTED
    assert attn(Hq=3, Hkv=2) == ARG
    assert attn(Q=0) == ARG and attn(Q=17) == ARG and attn(Scap=2) == ARG and attn(ns=0) == ARG and attn(B=-1) == ARG
    assert attn(mask=p, Sp=21) == ARG and attn(mask=p, Sp=-1) == ARG
    for name in ("q", "k", "v", "base", "out", "ws"):
        assert attn(**{name: None}) == ARG, name
    for name in ("q", "k", "v"):
        assert attn(**{name: p + 8}) == ALIGN, name
    for name in STRIDES:
        assert attn(**{name: 132}) == ALIGN, name
    assert attn(D=64, qsb=W + 4) == UNSUPPORTED and attn(Q=0, q=p + 8) == ARG          # the shape checks come first
    assert attn(B=0) == 0


def test_verify_split_count():
    L = _lib.lib()
    for B, Q, Hkv, Scap in ((4, 4, 8, 2081), (2, 8, 8, 2100), (1, 16, 8, 2064), (2, 5, 2, 70), (1, 1, 1, 130), (0, 4, 8, 100)):
        assert L.mm_attn_decode_verify_splits(B, Q, Hkv, Scap) == L.mm_attn_decode_shared_splits(B, Q, Hkv, Scap), (B, Q, Hkv, Scap)
    assert L.mm_attn_decode_verify_splits(4, 4, 8, 2081) == 16 and L.mm_attn_decode_verify_splits(1, 1, 1, 130) == 3


def test_new_kernels_use_no_scratch():
    path, attn = os.path.join(BUILD, "mm_lookup.o.resources.txt"), os.path.join(BUILD, "mm_attn.o.resources.txt")
    if not os.path.exists(path) or not os.path.exists(attn):
        pytest.skip("library not built in this tree (python multimeditron_amd/csrc/build.py)")
    ks = _kernels(path)
    want = {"lookup_draft_kernel", "kv_append_at_kernel", "lookup_accept_kernel"}
    assert len(ks) == 3 and {k for k in want for name, _ in ks if k in name} == want, ks
    va = [(name, s) for name, s in _kernels(attn) if "attn_decode_verify128_kernel" in name]
    assert len(va) == 3, va                                 # G in {1, 2, 4}
    for name, scratch in ks + va:
        assert scratch == 0, f"{name}: {scratch} bytes/lane of scratch"
