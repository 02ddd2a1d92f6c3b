"""Sampling without a GPU: the fp64 restatement of mm_sample's contract (tests/sampling_ref.py) against transformers' warpers,
its tie and -inf rules, mm_sample's argument checks before any launch, and the sampler kernels' scratch use."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import sampling_ref as S

BUILD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multimeditron_amd", "csrc", "build")


def _hf_kept(x, top_k, top_p, min_p):
    tr = pytest.importorskip("transformers")
    from transformers.generation.logits_process import MinPLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = torch.tensor(x, dtype=torch.float64)[None]
    ids = torch.zeros((1, 1), dtype=torch.long)
    if top_k:
        s = TopKLogitsWarper(top_k)(ids, s)
    if top_p < 1.0:
        s = TopPLogitsWarper(top_p)(ids, s)
    if min_p > 0.0:
        s = MinPLogitsWarper(min_p)(ids, s)
    del tr
    return torch.isfinite(s[0]).numpy()


@pytest.mark.parametrize("cfg", [(5, 1.0, 0.0), (50, 1.0, 0.0), (0, 0.9, 0.0), (0, 0.5, 0.0), (0, 1.0, 0.05), (40, 0.8, 0.0),
                                 (100, 0.95, 0.02)])
def test_contract_matches_transformers_warpers(cfg):
    top_k, top_p, min_p = cfg
    rng = np.random.default_rng(1 + top_k)
    for trial in range(8):
        V = int(rng.integers(200, 3000))
        logits = np.unique((rng.standard_normal(V) * rng.uniform(0.5, 4.0)).astype(np.float32))     # tie-free
        logits = logits[rng.permutation(logits.shape[0])]
        x = S.scaled(logits, 1.0)
        ref = S.contract_row(logits, 1.0, top_k, np.float32(top_p), np.float32(min_p), u=0.5)
        hf = _hf_kept(x.astype(np.float64), top_k, float(np.float32(top_p)), float(np.float32(min_p)))
        if ref["near_keep"]:
            continue
        assert np.array_equal(ref["kept"], hf), (cfg, trial)


def test_contract_ties_and_minus_inf():
    x = np.array([1.0, 3.0, 2.0, 3.0, 2.0, 2.0, -np.inf, 0.5], dtype=np.float32)
    # top-k = 3: the 3rd largest value is 2.0 -> every 2.0 is kept with the two 3.0
    r = S.contract_row(x, 1.0, top_k=3)
    assert r["thresh"] == 2.0 and r["kept"].tolist() == [False, True, True, True, True, True, False, False]
    # top-k = 2: the two tied maxima only
    r = S.contract_row(x, 1.0, top_k=2)
    assert r["thresh"] == 3.0 and r["kept"].sum() == 2
    # top-p: ties are decided by value -- the tied maxima are kept together even when one of them alone reaches top_p
    r = S.contract_row(x, 1.0, top_p=1e-6)
    assert r["kept"].tolist() == [False, True, False, True, False, False, False, False]
    # -inf is never drawn, whatever u
    for u in np.linspace(0.0, 1.0 - 2**-24, 257):
        r = S.contract_row(x, 1.0, top_k=8, u=u)
        assert x[r["tok"]] != -np.inf and r["kept"][r["tok"]]
    # top-k >= number of finite entries keeps -inf (threshold -inf) but still draws a finite one
    x2 = x.copy()
    x2[0] = -np.inf
    r = S.contract_row(x2, 1.0, top_k=7, u=1.0 - 2**-24)
    assert r["thresh"] == -np.inf and r["kept"].all() and r["tok"] == 7
    # the draw: smallest index whose cumulative kept mass exceeds t
    w = np.exp(x.astype(np.float64) - 3.0)
    w[6] = 0
    cum = np.cumsum(w)
    for u in (0.0, 0.3, 0.77, 0.999):
        assert S.contract_row(x, 1.0, u=u)["tok"] == int(np.searchsorted(cum, u * cum[-1], side="right"))
    # -0 and +0 are one value
    r = S.contract_row(np.array([-0.0, 0.0, -1.0], dtype=np.float32), 1.0, top_k=1)
    assert r["kept"].tolist() == [True, True, False]


def test_python_philox_known_answer():
    # Random123's published known-answer vectors for Philox4x32-10 (counter, key) -> output
    x, y, z, w = S.philox4x32_10(np.array([0], dtype=np.uint64), 0, 0)
    assert [int(x[0]), int(y[0]), int(z[0]), int(w[0])] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    c = 0x243F6A88 | (0x85A308D3 << 32)
    x, y, z, w = S.philox4x32_10(np.array([c], dtype=np.uint64), 0x13198A2E | (0x03707344 << 32), 0xA4093822 | (0x299F31D0 << 32))
    assert [int(x[0]), int(y[0]), int(z[0]), int(w[0])] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_argument_validation_without_launch():
    from multimeditron_amd import _lib
    L = _lib.lib()
    assert L.mm_version() >= 101
    nb = ctypes.c_int64(0)
    assert L.mm_sample_ws_bytes(4, 128258, ctypes.byref(nb)) == 0 and nb.value > 0
    assert L.mm_sample_ws_bytes(-1, 128258, ctypes.byref(nb)) == -1
    assert L.mm_sample_ws_bytes(4, 0, ctypes.byref(nb)) == -1
    L.mm_sample_ws_bytes(4, 1000, ctypes.byref(nb))
    ws_bytes = nb.value
    fake = 1 << 20                                   # never dereferenced: every call below is rejected before a launch
    good = dict(dtype=0, rows=4, V=1000, ld=1000, T=0.7, k=50, p=0.9, mp=0.05, ws=ws_bytes)

    def run(**kw):
        a = dict(good, **kw)
        return L.mm_sample(a["dtype"], fake, a["rows"], a["V"], a["ld"], a["T"], a["k"], a["p"], a["mp"], 1, 0, fake, None, fake,
                           a["ws"], None)
    for bad in (dict(T=0.0), dict(T=-1.0), dict(T=float("nan")), dict(k=-1), dict(p=0.0), dict(p=1.5), dict(p=float("nan")),
                dict(p=-0.1), dict(mp=-0.01), dict(mp=1.5), dict(mp=float("nan")), dict(ld=999), dict(rows=-1),
                dict(ws=ws_bytes - 1), dict(dtype=7), dict(V=0)):
        assert run(**bad) == -1, bad
    assert L.mm_sample_uniforms(0, 0, -1, fake, None) == -1
    assert L.mm_sample_uniforms(0, 0, 4, None, None) == -1


def test_sampler_kernels_use_no_scratch():
    path = os.path.join(BUILD, "mm_sample.o.resources.txt")
    if not os.path.exists(path):
        pytest.skip("library not built in this tree (python multimeditron_amd/csrc/build.py)")
    import re
    seen = {}
    name = None
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and name:
            seen[name] = int(m.group(1))
    for k in ("sample_max_kernel", "sample_hist_kernel", "sample_mass_kernel", "sample_draw_kernel", "sample_uniforms_kernel"):
        hits = [n for n in seen if k in n]
        assert hits, k
        assert all(seen[n] == 0 for n in hits), {n: seen[n] for n in hits}


def test_generate_rejects_bad_sampling_arguments():
    """generate() validates the sampler's arguments before touching the model (ValueError, nothing launched)."""
    from multimeditron_amd.model.model import MultiModalModelForCausalLM
    m = MultiModalModelForCausalLM.__new__(MultiModalModelForCausalLM)
    for bad in (dict(top_k=-1), dict(top_k=2.5), dict(top_p=0.0), dict(top_p=1.01), dict(min_p=-0.1), dict(min_p=2.0),
                dict(seed=-3), dict(seed=1.5)):
        with pytest.raises(ValueError):
            m.generate({}, max_new_tokens=4, do_sample=True, **bad)
