"""Beam search (CPU): tests/beam_ref.py -- the fp64 restatement every GPU test of mm_beam_step is held to -- against transformers'
own generate(num_beams, do_sample=False, length_penalty, early_stopping) on a tiny random fp32 Llama; the new entry points declared,
exported and refusing what they cannot run before any launch; and the build's resource remarks of the new kernels: no scratch."""
import ctypes
import itertools
import os
import re

import pytest
import torch

from multimeditron_amd import _lib
from tests import beam_ref as BR

BUILD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multimeditron_amd", "csrc", "build")
ARG, ALIGN = -1, -2
BF16, F32 = 0, 1


# ---- the reference against transformers -----------------------------------------------------------------------------------------
T_NEW, EOS = 8, 5
# (seed, prompts): two prompts that have to close together (the call runs to max_new_tokens; hypotheses end on eos on the way), and
# one prompt alone (the call is done early)
SETUPS = {"two": (3, [[1, 7, 9, 11], [1, 3, 20, 2]]), "one": (7, [[1, 7, 9, 11]])}


@pytest.fixture(scope="module")
def hf():
    tf = pytest.importorskip("transformers")
    out = {}
    for name, (seed, prompts) in SETUPS.items():
        torch.manual_seed(seed)
        cfg = tf.LlamaConfig(vocab_size=24, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2,
                             num_key_value_heads=2, max_position_embeddings=64, initializer_range=0.05, eos_token_id=EOS,
                             pad_token_id=EOS, bos_token_id=1)
        out[name] = (tf.LlamaForCausalLM(cfg).float().eval(), torch.tensor(prompts))
    return out


def _reference(hf, setup, es, lp, n, nrs):
    m, prompts = hf[setup]
    B = prompts.shape[0]

    def lp_fn(i, seqs):
        rows = []
        for b in range(B):
            for s in (seqs[b][:1] if i == 0 else seqs[b]):
                rows.append(torch.cat([prompts[b], torch.tensor(s if i else [], dtype=torch.long)]))
        with torch.no_grad():
            logits = m(input_ids=torch.stack(rows)).logits[:, -1].float()
        return torch.log_softmax(logits, dim=-1).double()           # HF's own fp32 log-probabilities

    return BR.search(lp_fn, B, n, T_NEW, EOS, lp, es, nrs)


HF_CASES = [(su, es, lp, n, nrs) for su, es, lp, n in itertools.product(sorted(SETUPS), (False, True, "never"), (0.0, 1.0, 2.0), (2, 4))
            for nrs in (1, n)]


@pytest.mark.parametrize("setup,es,lp,n,nrs", HF_CASES, ids=[f"{c[0]}-es{c[1]}-lp{c[2]:g}-n{c[3]}-nrs{c[4]}" for c in HF_CASES])
def test_reference_is_transformers_beam_search(hf, setup, es, lp, n, nrs):
    m, prompts = hf[setup]
    B, Sp = prompts.shape
    ids, scores, steps = _reference(hf, setup, es, lp, n, nrs)
    with torch.no_grad():
        out = m.generate(input_ids=prompts, attention_mask=torch.ones_like(prompts), num_beams=n, do_sample=False, length_penalty=lp,
                         early_stopping=es, num_return_sequences=nrs, max_new_tokens=T_NEW, output_scores=True,
                         return_dict_in_generate=True, pad_token_id=EOS, eos_token_id=EOS)
    got = out.sequences[:, Sp:]
    assert got.shape[0] == B * nrs == len(ids)
    n_out = max(len(s) for s in ids)
    assert got.shape[1] == n_out
    for r, s in enumerate(ids):
        assert got[r].tolist() == s + [EOS] * (n_out - len(s)), (r, got[r].tolist(), s)
    torch.testing.assert_close(out.sequences_scores.double(), torch.tensor(scores, dtype=torch.float64), rtol=1e-5, atol=1e-5)


def test_the_cases_finish_early_and_run_out(hf):
    runs = [_reference(hf, su, es, lp, n, n) for su, es, lp, n, nrs in HF_CASES if nrs == n]
    assert any(steps < T_NEW for _, _, steps in runs), "no case was done before max_new_tokens"
    assert any(steps == T_NEW for _, _, steps in runs), "no case ran to max_new_tokens"
    assert any(len(s) < T_NEW and s[-1] == EOS for ids, _, _ in runs for s in ids), "no hypothesis finished on eos"
    assert any(len(s) == T_NEW and s[-1] != EOS for ids, _, _ in runs for s in ids), "no hypothesis ran to max_new_tokens"


def test_reference_ties_and_nearness():
    """ties go to the smaller flat index; an exact tie inside a row is not near, and neither is one across two rows of equal score
    whose log-probability rows are bit-equal (fp32 keeps both equal); any other tie across rows is"""
    p = BR.Prompt(2)
    lp = BR.log_probs(torch.tensor([[1.0, 3.0, 3.0, 0.0, 3.0, -float("inf")]]))
    r = BR.step(p, lp, 0, 4, eos=9, tau=1e-4)
    assert r["tok"] == [1, 2] and r["parent"] == [0, 0] and not r["near"]
    p = BR.Prompt(2)
    p.s, p.seq = [-1.0, -1.0], [[1], [2]]
    rows = BR.log_probs(torch.tensor([[0.0, 5.0, 1.0, 1.0, 0.5, 0.2], [0.0, 5.0, 1.0, 1.0, 0.5, 0.2]]))
    r = BR.step(p.copy(), rows, 1, 4, eos=9, tau=1e-4)
    assert r["tok"] == [1, 1] and r["parent"] == [0, 1] and not r["near"]
    # the same values from rows that are not bit-equal (the tail swapped: another sum), and bit-equal rows under different scores
    swapped = BR.log_probs(torch.tensor([[0.0, 5.0, 1.0, 1.0, 0.5, 0.2], [0.0, 5.0, 1.0, 1.0, 0.2, 0.5]]))
    r = BR.step(p.copy(), swapped, 1, 4, eos=9, tau=1e-4)
    assert r["tok"] == [1, 1] and sorted(r["parent"]) == [0, 1] and r["near"]
    q = p.copy()
    q.s = [-1.0, -1.0 - 1e-6]
    r = BR.step(q, rows, 1, 4, eos=9, tau=1e-4)
    assert r["tok"] == [1, 1] and r["parent"] == [0, 1] and r["near"]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
NEW = ("mm_attn_decode_beam", "mm_beam_ws_bytes", "mm_beam_state_bytes", "mm_beam_state_layout", "mm_beam_step", "mm_beam_finish")


def test_symbols_declared_and_exported():
    protos = _lib.parse_header()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in protos, f"include/mm_hip.h does not declare {name}"
        assert hasattr(L, name), f"libmmhip.so does not export {name}"
    assert len(protos["mm_attn_decode_beam"][1]) == 35 and len(protos["mm_beam_step"][1]) == 17


def test_beam_refusals_come_before_any_launch():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 20)
    p = (ctypes.addressof(buf) + 15) & ~15
    nb = ctypes.c_int64(0)
    assert L.mm_beam_ws_bytes(3, 5, 1003, ctypes.byref(nb)) == 0 and nb.value > 0
    ws_bytes = nb.value
    assert L.mm_beam_state_bytes(3, 5, 8, ctypes.byref(nb)) == 0 and nb.value > 0
    st_bytes = nb.value
    assert max(ws_bytes, st_bytes) < (1 << 20) - 16
    off = (ctypes.c_int64 * 11)()
    assert L.mm_beam_state_layout(3, 5, 8, off) == 0
    assert list(off) == sorted(off) and off[0] == 0 and all(o % 16 == 0 for o in off) and off[10] + 4 <= st_bytes
    for f in (L.mm_beam_ws_bytes, ):
        assert f(3, 0, 1003, ctypes.byref(nb)) == ARG and f(3, 17, 1003, ctypes.byref(nb)) == ARG and f(3, 5, 9, ctypes.byref(nb)) == ARG
        assert f(0, 5, 1003, ctypes.byref(nb)) == ARG and f(3, 5, 1003, None) == ARG
    assert L.mm_beam_state_bytes(3, 17, 8, ctypes.byref(nb)) == ARG and L.mm_beam_state_bytes(3, 5, 0, ctypes.byref(nb)) == ARG
    assert L.mm_beam_state_layout(3, 0, 8, off) == ARG and L.mm_beam_state_layout(3, 5, 8, None) == ARG

    def step(dtype=BF16, logits=p, B=3, n=5, V=1003, ld=1024, i=0, T=8, eos=2, lp=1.0, es=0, state=p, sb=st_bytes, ws=p, wb=ws_bytes, nxt=p):
        return L.mm_beam_step(dtype, logits, B, n, V, ld, i, T, eos, ctypes.c_float(lp), es, state, sb, ws, wb, nxt, None)

    assert step(n=0) == ARG and step(n=17) == ARG and step(B=0) == ARG
    assert step(V=9) == ARG and step(V=(1 << 24) + 1, ld=(1 << 24) + 8) == ARG and step(ld=1002) == ARG
    assert step(i=-1) == ARG and step(i=8) == ARG and step(T=0) == ARG
    assert step(es=3) == ARG and step(es=-1) == ARG and step(lp=float("inf")) == ARG and step(lp=float("nan")) == ARG
    assert step(dtype=2) == ARG
    for name in ("logits", "state", "ws", "nxt"):
        assert step(**{name: None}) == ARG, name
    assert step(sb=st_bytes - 1) == ARG and step(wb=ws_bytes - 1) == ARG
    assert step(state=p + 8) == ALIGN and step(ws=p + 4) == ALIGN
    assert step(n=17, state=p + 8) == ARG                         # the shape's code comes first

    def finish(state=p, sb=st_bytes, B=3, n=5, T=8, nrs=2, ids=p, scores=p, lens=p):
        return L.mm_beam_finish(state, sb, B, n, T, nrs, 2, ids, scores, lens, None)

    assert finish(nrs=0) == ARG and finish(nrs=6) == ARG and finish(n=17) == ARG and finish(sb=st_bytes - 1) == ARG
    for name in ("state", "ids", "scores", "lens"):
        assert finish(**{name: None}) == ARG, name
    assert finish(state=p + 8) == ALIGN


def test_attn_decode_beam_refusals_come_before_any_launch():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    W = 4 * 128

    def attn(q=p, B=2, n=3, Ss=2, Hq=2, D=128, anc=p, ld=6, ns=1, qsb=W):
        return L.mm_attn_decode_beam(BF16, q, p, p, p, p, B, n, 5, Ss, Hq, 1, D, qsb, 128, 8 * 128, 128, 128, 8 * 128, 128, 128, 4 * 128, 128, 128,
                                     4 * 128, 128, 128, None, ctypes.c_float(0.1), p, p, ns, anc, ld, None)

    assert attn(anc=None) == ARG and attn(ld=5) == ARG
    assert attn(D=64) == -3 and attn(Hq=8) == -3 and attn(n=0) == ARG and attn(Ss=0) == ARG and attn(ns=0) == ARG
    assert attn(q=p + 8) == ALIGN and attn(qsb=W + 4) == ALIGN
    assert attn(B=0) == 0


# ---- the build ------------------------------------------------------------------------------------------------------------------
def _remarks(path):
    out, cur = {}, None
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and cur is not None:
            cur["scratch"] = int(m.group(1))
    return out


@pytest.mark.parametrize("fname,needle,count", [("mm_attn.o.resources.txt", "attn_decode_beam128_kernel", 3),
                                                ("mm_beam.o.resources.txt", "beam_", 5)])
def test_new_kernels_use_no_scratch(fname, needle, count):
    path = os.path.join(BUILD, fname)
    if not os.path.exists(path):
        pytest.skip("library not built in this tree (python multimeditron_amd/csrc/build.py)")
    new = {n: r for n, r in _remarks(path).items() if needle in n}
    assert len(new) == count, sorted(new)
    for name, r in sorted(new.items()):
        assert r["scratch"] == 0, f"{name}: {r['scratch']} bytes/lane of scratch"
