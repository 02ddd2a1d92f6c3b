"""mm_logits_process on the GPU against tests/logits_ref.py, bit for bit on out[:, :V]: both dtypes, one / several / sixteen rows,
vocabularies below, just above and far above one chunk, padded rows with NaN poison behind V (the output's pad must come back
untouched), every rule on and off, histories that are empty, shorter than the n-gram, full of duplicates, on the chunk edges and out
of range, a different prompt length per row; the history the kernel keeps over steps 0 .. 5; equal bits on a second launch; no
history at all (NULL)."""
import numpy as np
import pytest
import torch

from multimeditron_amd import kernels as K
from multimeditron_amd._lib import call
from tests import logits_ref as LR

pytestmark = pytest.mark.gpu

SENTINEL = -7
POISON = 0x7FC00ABC            # a NaN with a payload: "unchanged" is a comparison of bits


def _logits(rng, rows, V, ld, dtype):
    """[rows, ld] on the device, NaN behind V; the fp32 values of its first V columns on the host"""
    x = (rng.standard_normal((rows, V)) * 4).astype(np.float32)
    k = max(1, V // 16)
    for r in range(rows):
        x[r, rng.integers(0, V, k)] = 0.0
        x[r, rng.integers(0, V, k)] = -0.0
        x[r, rng.integers(0, V, k)] = -np.inf
    t = torch.full((rows, ld), float("nan"), dtype=dtype)
    t[:, :V] = torch.from_numpy(x).to(dtype)
    return t.cuda(), t[:, :V].float().numpy()


def _edges(V):
    e = {0, 1, V - 2, V - 1}
    for c in range(LR.LCHUNK, V + 2, LR.LCHUNK):
        e |= {c - 1, c, c + 1}
    return sorted(t for t in e if 0 <= t < V)


def _history(kind, rng, V, g, step):
    """one row's history of at least `step` ids"""
    e = _edges(V)
    if kind == "empty":
        h = []
    elif kind == "one":
        h = [V - 1]
    elif kind in ("g-2", "g-1", "g"):
        h = [int(t) for t in rng.integers(0, 2, max(0, g - {"g-2": 2, "g-1": 1, "g": 0}[kind]))]
    elif kind == "abc":                                        # 2600 ids over three: duplicates and matching n-grams everywhere
        h = [(0, V // 2, V - 1)[t] for t in rng.integers(0, 3, 2600)]
    elif kind == "edges":                                      # every chunk edge +-1, twice: the tail matches and bans edge ids
        k = int(rng.integers(1, len(e)))
        h = e + e[:k]
    elif kind == "outside":                                    # -1 and V are ignored, the ids beside them are not
        h = [0, -1, V, V - 1, 5, -1, V, 7, 0, -1, V, 2 ** 31 - 1, -2 ** 31, 0, -1, V]
    else:
        h = [int(t) for t in rng.integers(0, V, int(rng.integers(3, 40)))]
    while len(h) < step:
        h.append(int(rng.integers(0, min(V, 3))))
    return h


KINDS = ["empty", "one", "g-2", "g-1", "g", "abc", "edges", "outside", "random"]


def _launch(x_dev, V, hists, step, p, g, mn, eos, sup, ld_out, room=3, keep_hist=True):
    """one call on histories given as lists: the last id of a row comes in through last_ids when step > 0.
    -> (out [rows, ld_out] on the host, hist after the call, what hist must hold, hist before)"""
    rows = x_dev.shape[0]
    out = torch.full((rows, ld_out), 0.0, dtype=torch.float32).view(torch.int32).fill_(POISON).view(torch.float32).cuda()
    hist = plen = last = want_hist = before = None
    max_plen = 0
    if keep_hist:
        plens = [len(h) - step for h in hists]
        max_plen = max(plens)
        ld_hist = max_plen + step + room
        hb = np.full((rows, ld_hist), SENTINEL, dtype=np.int64)
        want_hist = hb.copy()
        for r, h in enumerate(hists):
            stored = len(h) - (1 if step > 0 else 0)           # the newest id is not in hist yet
            hb[r, :stored] = h[:stored]
            want_hist[r, :len(h)] = h
        before = hb.astype(np.int32)
        hist = torch.from_numpy(before.copy()).cuda()
        want_hist = want_hist.astype(np.int32)
        plen = torch.tensor(plens, dtype=torch.int32).cuda()
        if step > 0:
            last = torch.tensor([h[-1] for h in hists], dtype=torch.int64).cuda()
    s = torch.tensor(sup, dtype=torch.int32).cuda() if len(sup) else None
    call("mm_logits_process", K.dt(x_dev), x_dev.data_ptr(), rows, V, x_dev.stride(0), step, None if last is None else last.data_ptr(),
         None if hist is None else hist.data_ptr(), 0 if hist is None else hist.stride(0), None if plen is None else plen.data_ptr(),
         max_plen, float(p), int(g), int(mn), int(eos), None if s is None else s.data_ptr(), len(sup), out.data_ptr(), ld_out,
         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu(), None if hist is None else hist.cpu().numpy(), want_hist, before


def _check(out, V, x_host, hists, step, **kw):
    want = LR.process(x_host, hists, step, **kw)
    got = out[:, :V].numpy()
    if not LR.same_bits(got, want):
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        r, v = bad[0]
        raise AssertionError(f"{len(bad)} entries differ; first: row {r} id {v}: got {got[r, v]!r}, want {want[r, v]!r}, logit {x_host[r, v]!r}")
    pad = out[:, V:].contiguous().view(torch.int32)
    assert bool((pad == POISON).all()), "the output's pad columns were written"
    assert bool(np.isfinite(want).any(axis=1).all()), "a row of the test has no finite score left"


def _suppress(rng, V, n, eos):
    if n == 0:
        return []
    if n == 1:
        return [eos]
    s = [int(t) for t in rng.integers(0, V, n - 6)] + [eos, eos, -1, V, 0, V - 1]
    s[3] = s[2]
    return s


# every dtype x rows x V, the other settings walking through their values
GRID = [(dt_, rows, V) for dt_ in (torch.bfloat16, torch.float32) for rows in (1, 3, 16) for V in (1003, 4099, 128258)]


@pytest.mark.parametrize("n", range(len(GRID)), ids=[f"{str(d).split('.')[-1]}-r{r}-V{v}" for d, r, v in GRID])
def test_rows_match_the_reference_bitwise(n):
    dtype, rows, V = GRID[n]
    rng = np.random.default_rng(100 + n)
    p = (1.3, 0.7, 1.0)[n % 3]
    g = (3, 0, 1, 2, 5)[n % 5]
    step = (0, 1, 4)[(n // 2) % 3]
    mn = (step + 1, step, 0)[n % 3]
    pad = (0, 5, 64)[(n // 3) % 3]               # 0: rows of V entries (odd V: the scalar path); 64: aligned rows of the padded width
    ld = V + pad if pad < 64 else (V + 63) // 64 * 64 + 64
    ld_out = V + (3, 0, 6)[n % 3] if pad < 64 else (V + 63) // 64 * 64
    eos = int(rng.integers(0, V))
    x_dev, x_host = _logits(rng, rows, V, ld, dtype)
    kinds = [k for k in KINDS if step == 0 or k != "empty"]
    hists = [_history(kinds[(n + r) % len(kinds)], rng, V, g, step) for r in range(rows)]
    sup = _suppress(rng, V, (0, 1, 300)[(n // 6) % 3], eos)
    out, hist, want_hist, _ = _launch(x_dev, V, hists, step, p, g, mn, eos, sup, ld_out)
    _check(out, V, x_host, hists, step, p=p, g=g, min_new_tokens=mn, eos=eos, suppress=sup)
    assert np.array_equal(hist, want_hist)


@pytest.mark.parametrize("p", [1.0, 0.7, 1.3])
@pytest.mark.parametrize("g", [0, 1, 2, 3, 5])
def test_every_penalty_and_ngram_size_on_every_kind_of_history(p, g):
    """V = 4099 (two chunks, the second of three entries), 18 rows: every kind of history at step 0 and at step 2, bf16"""
    V, rng = 4099, np.random.default_rng(int(p * 10) * 7 + g)
    for step in (0, 2):
        kinds = [k for k in KINDS if step == 0 or k != "empty"] * 2
        hists = [_history(k, rng, V, g, step) for k in kinds]
        x_dev, x_host = _logits(rng, len(hists), V, V + 5, torch.bfloat16)
        eos = V - 1
        for mn, sup in ((0, []), (step + 1, _suppress(rng, V, 300, eos))):
            out, hist, want_hist, _ = _launch(x_dev, V, hists, step, p, g, mn, eos, sup, V + 1)
            _check(out, V, x_host, hists, step, p=p, g=g, min_new_tokens=mn, eos=eos, suppress=sup)
            assert np.array_equal(hist, want_hist)


def test_chunk_edges_of_the_large_vocabulary():
    """V = 128 258: ids on both sides of all 31 chunk boundaries, 0 and V - 1, penalised and banned; fp32 and bf16, aligned rows"""
    V, rng = 128258, np.random.default_rng(5)
    e = _edges(V)
    assert len(e) >= 3 * 31 + 2 and 4095 in e and 4096 in e and 4097 in e and 126976 in e and V - 1 in e
    for dtype in (torch.float32, torch.bfloat16):
        x_dev, x_host = _logits(rng, 2, V, 128320, dtype)
        hists = [e + e[:40] + [e[40]], list(reversed(e))]
        for g in (1, 2):
            out, _, _, _ = _launch(x_dev, V, hists, 1, 1.3, g, 2, V - 1, e[::2] + [4096, 4096], 128320)
            _check(out, V, x_host, hists, 1, p=1.3, g=g, min_new_tokens=2, eos=V - 1, suppress=e[::2] + [4096, 4096])
            if g == 1:
                assert bool(torch.isinf(out[0, e]).all())


def test_history_is_kept_over_the_steps():
    """steps 0 .. 5 in sequence through K.logits_process: every step sees the ids of the steps before it, hist ends up holding exactly
    the appended ids, the sentinel behind them and the pad ids in front untouched"""
    V, rows, rng = 4099, 3, np.random.default_rng(9)
    prompt = torch.tensor([[7, 7, 4096, 4098, 7, 7], [0, 9, 9, 9, 9, 0], [5, 6, 5, 6, 5, 6]])
    mask = torch.tensor([[0, 0, 1, 1, 1, 1], [1, 1, 1, 0, 1, 1], [1, 1, 1, 1, 1, 1]])
    visible = [[4096, 4098, 7, 7], [0, 9, 9, 9, 0], [5, 6, 5, 6, 5, 6]]
    st = K.LogitsState(rows, V, "cuda", 1.3, 2, 3, [1, 2], prompt_ids=prompt.cuda(), prompt_mask=mask.cuda(), room=8)
    assert st.hist.dtype == torch.int32 and st.hist.shape == (rows, 14) and st.plen.tolist() == [4, 5, 6] and st.max_plen == 6
    for r in range(rows):
        assert st.hist[r, :len(visible[r])].tolist() == visible[r]
    st.hist[:, 6:] = SENTINEL
    start = st.hist.cpu().numpy().copy()
    emitted = [[7, 4096, 7, 4096, 4098], [9, 0, 9, -1, 4099], [5, 6, 5, 6, 5]]           # what the steps 0 .. 4 "chose"
    last = torch.zeros(rows, dtype=torch.int64, device="cuda")
    for step in range(6):
        x_dev, x_host = _logits(rng, rows, V, 4160, torch.bfloat16)
        if step > 0:
            last.copy_(torch.tensor([emitted[r][step - 1] for r in range(rows)]))
        y = K.logits_process(x_dev, st, step, last, 4098)
        assert y.shape == (rows, V) and y.dtype == torch.float32 and y.data_ptr() == st.out.data_ptr()
        hists = [visible[r] + emitted[r][:step] for r in range(rows)]
        want = LR.process(x_host, hists, step, p=1.3, g=2, min_new_tokens=3, eos=4098, suppress=[1, 2])
        assert LR.same_bits(y.cpu().numpy(), want), step
    want_hist = start.copy()
    for r in range(rows):
        want_hist[r, len(visible[r]):len(visible[r]) + 5] = emitted[r]
    assert np.array_equal(st.hist.cpu().numpy(), want_hist)


def test_state_repeats_the_prompt_per_sample():
    prompt = torch.tensor([[3, 1, 2], [4, 4, 4]]).cuda()
    mask = torch.tensor([[0, 1, 1], [1, 1, 1]]).cuda()
    st = K.LogitsState(6, 50, "cuda", 1.0, 3, prompt_ids=prompt, prompt_mask=mask, samples=3, room=2)
    assert st.plen.tolist() == [2, 2, 2, 3, 3, 3] and st.hist.shape == (6, 5) and st.hist.is_contiguous()
    assert st.hist[:, :3].tolist() == [[1, 2, -1]] * 3 + [[4, 4, 4]] * 3
    off = K.LogitsState(2, 50, "cuda", min_new_tokens=2, suppress=[3])
    assert off.hist is None and off.plen is None and off.suppress.tolist() == [3]


def test_two_launches_give_the_same_bits():
    V, rng = 128258, np.random.default_rng(11)
    x_dev, _ = _logits(rng, 4, V, 128320, torch.bfloat16)
    hists = [_history("abc", rng, V, 3, 1) for _ in range(4)]
    a, ha, want_hist, _ = _launch(x_dev, V, hists, 1, 1.3, 3, 0, 0, [5, 6], 128320)
    b, hb, _, _ = _launch(x_dev, V, hists, 1, 1.3, 3, 0, 0, [5, 6], 128320)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and np.array_equal(ha, hb) and np.array_equal(ha, want_hist)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_without_a_history(dtype):
    """hist = plen = last_ids = NULL with p = 1 and g = 0: minimum length and suppression only"""
    V, rng = 4099, np.random.default_rng(13)
    x_dev, x_host = _logits(rng, 3, V, V + 1, dtype)
    for step, mn in ((0, 1), (1, 1), (4, 9)):
        out, hist, _, _ = _launch(x_dev, V, [[]] * 3, step, 1.0, 0, mn, 4096, [0, 4098, 4098], V + 2, keep_hist=False)
        assert hist is None
        _check(out, V, x_host, [[]] * 3, step, p=1.0, g=0, min_new_tokens=mn, eos=4096, suppress=[0, 4098, 4098])
    # all four off: the fp32 copy of the logits
    out, _, _, _ = _launch(x_dev, V, [[]] * 3, 0, 1.0, 0, 0, 0, [], V, keep_hist=False)
    assert LR.same_bits(out.numpy(), x_host)
