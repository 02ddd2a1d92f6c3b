"""mm_logits_process without a GPU: the numpy restatement of its five rules (tests/logits_ref.py) agrees bit for bit with
transformers' RepetitionPenalty -> NoRepeatNGram -> MinNewTokensLength -> SuppressTokens processors on seeded random fp32 rows, and the
library refuses every bad argument before it launches anything."""
import math

import numpy as np
import pytest

from multimeditron_amd import _lib
from tests import logits_ref as LR


def _row(rng, V):
    x = (rng.standard_normal(V) * 3).astype(np.float32)
    k = max(1, V // 8)
    x[rng.integers(0, V, k)] = 0.0
    x[rng.integers(0, V, k)] = -0.0
    x[rng.integers(0, V, k)] = -np.inf
    x[rng.integers(0, V)] = 1.5                  # a finite score survives
    return x


def _cases():
    rng = np.random.default_rng(20240)
    out = []
    for n in range(360):
        V = (17, 33, 1003)[n % 3]
        A = (2, 3, V)[(n // 3) % 3]              # alphabet of the history: small ones repeat ids and n-grams
        p = (1.0, 1.3, 0.7)[(n // 9) % 3]
        g = (n // 27) % 5
        lens = [0, 1, g - 2, g - 1, g] + [int(t) for t in rng.integers(0, 21, 3)]
        L = max(0, lens[n % len(lens)])
        h = [int(t) for t in rng.integers(0, A, L)]
        step = int(rng.integers(0, L + 1))
        mn = (0, step, step + 1)[n % 3]
        eos = int(rng.integers(0, V))
        sup = [int(t) for t in rng.integers(0, V, (0, 1, 5)[(n // 2) % 3])]
        if len(sup) > 1:
            sup.append(sup[0])
        out.append((V, _row(rng, V), h, step, dict(p=p, g=g, min_new_tokens=mn, eos=eos, suppress=sup)))
    return out


def test_helper_matches_transformers_bit_for_bit():
    pytest.importorskip("transformers")
    cases = _cases()
    assert len(cases) >= 300
    seen_L, compared = set(), 0
    for V, x, h, step, kw in cases:
        got = LR.process_row(x, h, step, **kw)
        seen_L.add((kw["g"], len(h) - kw["g"]))
        if len(h) == 0:                          # transformers cannot gather from an empty history: rules 3 and 4 only
            want = x.copy()
            if step < kw["min_new_tokens"]:
                want[kw["eos"]] = -np.inf
            for t in kw["suppress"]:
                want[t] = -np.inf
        else:
            want = LR.hf_process_row(x, h, step, **kw)
            compared += 1
        assert LR.same_bits(got, want), (V, h, step, kw, np.nonzero(got.view(np.uint32) != want.view(np.uint32)))
    assert compared >= 250
    for g in (2, 3, 4):                          # histories of g-2, g-1 and g ids were among them
        assert {(g, -2), (g, -1), (g, 0)} <= seen_L


def test_helper_rules_by_hand():
    x = np.array([2.0, -2.0, -0.0, 0.0, -np.inf, 1.0, 3.0, 4.0], dtype=np.float32)
    y = LR.process_row(x, [0, 1, 2, 3, 4, 0, 0, -1, 8], 0, p=1.3)
    want = np.array([np.float32(2.0) / np.float32(1.3), np.float32(-2.0) * np.float32(1.3), -0.0, 0.0, -np.inf, 1.0, 3.0, 4.0], dtype=np.float32)
    assert LR.same_bits(y, want) and np.signbit(y[2]) and not np.signbit(y[3])
    # 2-gram ban: the tail is [5]; 5 was followed by 6 and by 7
    y = LR.process_row(x, [5, 6, 1, 5, 7, 5], 3, g=2)
    assert np.isinf(y[[6, 7]]).all() and LR.same_bits(np.delete(y, [6, 7]), np.delete(x, [6, 7]))
    # g = 1 bans every id of the history; L + 1 < g bans nothing
    assert np.nonzero(np.isinf(LR.process_row(x, [5, 6], 0, g=1)))[0].tolist() == [4, 5, 6]
    assert LR.same_bits(LR.process_row(x, [5, 5], 0, g=4), x)
    assert LR.same_bits(LR.process_row(x, [5, 5], 0, g=3), x) and np.isinf(LR.process_row(x, [5, 5, 5], 0, g=3)[5])
    y = LR.process_row(x, [], 2, min_new_tokens=3, eos=7, suppress=[0, 0, 9, -1])
    assert np.isinf(y[[0, 7]]).all() and y[6] == 3.0
    assert LR.process_row(x, [], 3, min_new_tokens=3, eos=7)[7] == 4.0


def test_kernel_uses_no_scratch():
    """the build's resource remarks (csrc/build.py keeps them beside every object): both instantiations, no scratch, 1 KiB of LDS"""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "build", "mm_logits.o.resources.txt")
    text = open(path).read()
    names = re.findall(r"Function Name: (\S*logits_process_kernel\S*)", text)
    assert len(names) == 2, names
    assert [int(t) for t in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)] == [0, 0]
    assert [int(t) for t in re.findall(r"LDS Size \[bytes/block\]: (\d+)", text)] == [1024, 1024]


def test_library_refuses_bad_arguments_without_a_launch():
    L = _lib.lib()
    P = 4096                                      # a non-NULL address that is never dereferenced: every call fails its checks first
    ok = dict(dtype=0, logits=P, rows=2, V=100, ld=104, step=1, last_ids=P, hist=P, ld_hist=64, plen=P, max_plen=32, p=1.2, g=3, mn=0,
              eos=5, suppress=P, n_suppress=2, out=2 * P, ld_out=100, stream=None)

    def rc(**kw):
        a = dict(ok, **kw)
        return L.mm_logits_process(a["dtype"], a["logits"], a["rows"], a["V"], a["ld"], a["step"], a["last_ids"], a["hist"], a["ld_hist"],
                                   a["plen"], a["max_plen"], a["p"], a["g"], a["mn"], a["eos"], a["suppress"], a["n_suppress"], a["out"],
                                   a["ld_out"], a["stream"])

    bad = [dict(p=0.0), dict(p=-1.0), dict(p=math.nan), dict(p=math.inf), dict(g=-1), dict(mn=-1), dict(step=-1),
           dict(mn=2, eos=100), dict(mn=2, eos=-1), dict(ld=99), dict(ld_out=99), dict(rows=-1), dict(n_suppress=-1),
           dict(max_plen=64), dict(step=33), dict(max_plen=-1), dict(logits=None), dict(out=None), dict(suppress=None), dict(hist=None),
           dict(plen=None), dict(hist=None, p=1.0), dict(hist=None, g=0), dict(plen=None, p=1.0, g=0), dict(last_ids=None),
           dict(out=P), dict(dtype=2), dict(V=0, ld=0, ld_out=0)]
    for kw in bad:
        assert rc(**kw) == -1, kw
    # rows = 0 is fine once the arguments are; so is a call that keeps no history, without last_ids
    assert rc(rows=0) == 0
    assert rc(rows=0, hist=None, plen=None, last_ids=None, p=1.0, g=0) == 0
    assert rc(rows=0, mn=2, eos=99, step=1) == 0 and rc(rows=0, mn=1, eos=100, step=1) == 0     # eos matters while step < min_new_tokens
    assert rc(rows=0, max_plen=63, step=1) == 0
