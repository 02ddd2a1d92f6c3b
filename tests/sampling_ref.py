"""The sampling contract of mm_sample (include/mm_hip.h) restated in numpy / fp64, a Python Philox4x32-10, and an oracle-driven
sampled generate().  A helper for tests/test_sampling_*.py, not a test module."""
import numpy as np
import torch

from oracle import ref_cpu as R

_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(call, offset, seed):
    """Philox4x32-10 of csrc/mm_common.h for an array of `call` counters: -> (x, y, z, w) uint64 arrays of 32-bit words."""
    c = np.asarray(call, dtype=np.uint64)
    offset, seed = int(offset) & (2**64 - 1), int(seed) & (2**64 - 1)
    c0, c1 = c & _M32, c >> np.uint64(32)
    c2 = np.full_like(c, offset & 0xFFFFFFFF)
    c3 = np.full_like(c, offset >> 32)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        h0, l0 = p0 >> np.uint64(32), p0 & _M32
        h1, l1 = p1 >> np.uint64(32), p1 & _M32
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def uniforms(seed, offset, rows):
    """u of the contract's step 5 for rows 0 .. rows-1 (float64, exact)."""
    x = philox4x32_10(np.arange(rows, dtype=np.uint64), offset, seed)[0]
    return (x >> np.uint64(8)).astype(np.float64) * 2.0**-24


def scaled(logits_row, temperature):
    """step 1's x in fp32: float(logit) / T with T rounded to fp32 (what crosses the C ABI), -0 -> +0."""
    x = np.asarray(logits_row, dtype=np.float32) / np.float32(temperature)
    x = x.astype(np.float32)
    x[x == 0] = 0.0
    return x


def contract_row(logits_row, temperature, top_k=0, top_p=1.0, min_p=0.0, u=0.0, tol=1e-5):
    """The contract for one row in fp64.  Returns dict(tok, thresh, kept, near_keep, near_draw): near_keep / near_draw tell that
    a top-p / min-p decision or the draw lies within tol of its boundary (tol * Z_K for top-p, tol for min-p's w, tol * Z for
    the draw), where a fixed-point or fp32 computation may legitimately decide the other way."""
    x = scaled(logits_row, temperature)
    V = x.shape[0]
    xd = x.astype(np.float64)
    m = xd.max()
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.exp(xd - m)
    w[~np.isfinite(w)] = 0.0
    kept = np.ones(V, dtype=bool)
    near_keep = False
    top_p, min_p = float(np.float32(top_p)), float(np.float32(min_p))
    if 0 < top_k < V:
        xk = np.sort(x)[::-1][top_k - 1]
        kept &= x >= xk
    if top_p < 1.0:
        vals, inv = np.unique(-x[kept], return_inverse=True)       # distinct kept values, descending
        mass = np.bincount(inv, weights=w[kept], minlength=vals.shape[0])
        above = np.concatenate([[0.0], np.cumsum(mass)[:-1]])       # mass strictly above each distinct value
        zk = mass.sum()
        target = top_p * zk
        near_keep |= bool(np.any(np.abs(above - target) <= tol * zk))
        keep_val = above < target
        kk = np.zeros(V, dtype=bool)
        kk[np.flatnonzero(kept)] = keep_val[inv]
        kept = kk
    if min_p > 0.0:
        near_keep |= bool(np.any(np.abs(w[kept] - min_p) <= tol))
        kept &= w >= min_p
    wk = np.where(kept, w, 0.0)
    cum = np.cumsum(wk)
    Z = cum[-1]
    t = u * Z
    v = int(np.searchsorted(cum, t, side="right"))
    pos = np.flatnonzero(kept & (w > 0))
    if v >= V:
        v = int(pos[-1]) if pos.size else 0
    lo = cum[v - 1] if v > 0 else 0.0
    near_draw = bool(min(abs(t - lo), abs(cum[v] - t)) <= tol * Z)
    thr = x[kept].min() if kept.any() else np.float32(np.nan)
    return dict(tok=v, thresh=np.float32(thr), kept=kept, near_keep=near_keep, near_draw=near_draw)


def contract(logits2d, temperature, top_k=0, top_p=1.0, min_p=0.0, seed=0, offset=0, tol=1e-5):
    """contract_row for every row of a [rows, V] array, row r drawing with call r."""
    lg = np.asarray(logits2d, dtype=np.float32)
    u = uniforms(seed, offset, lg.shape[0])
    return [contract_row(lg[r], temperature, top_k, top_p, min_p, u[r], tol) for r in range(lg.shape[0])]


@torch.no_grad()
def sample_generate(w, batch, meta, max_new_tokens=8, temperature=0.7, top_k=0, top_p=1.0, min_p=0.0, seed=0, tol=1e-4):
    """generate(do_sample=True, top_k, top_p, min_p, seed) on the oracle's public functions: step i draws with Philox offset i,
    call = row.  Returns (ids [B, n], comparable [B, n] bool): a row stops being comparable after a step whose decisions lay
    within tol of a boundary (the device's logits differ from the oracle's by rounding)."""
    temperature = max(temperature, 1e-6)
    llm = meta["llm"]
    eos = meta["eos_token_idx"]
    nxt = R.multimodal_embed(w, batch, meta)
    mask = batch["attention_mask"]
    pos = batch["position_ids"]
    B, S = mask.shape
    cache = [None] * llm["num_hidden_layers"]
    finished = torch.zeros(B, dtype=torch.bool)
    live = np.ones(B, dtype=bool)
    toks, comp = [], []
    for i in range(max_new_tokens):
        if i > 0:
            pos = (S + i - 1) * torch.ones(B, 1, dtype=torch.long)
            mask = torch.cat([mask, torch.ones(B, 1, dtype=mask.dtype)], dim=-1)
        h = R.decoder_forward(w, nxt, mask, pos, llm, cache=cache)
        raw = torch.nn.functional.linear(h[:, -1, :], R.lm_head_weight(w, llm)).float().numpy()
        res = contract(raw, temperature, top_k, top_p, min_p, seed=seed, offset=i, tol=tol)
        tok = torch.tensor([r["tok"] for r in res], dtype=torch.int64)
        for b in range(B):
            if not bool(finished[b]) and (res[b]["near_keep"] or res[b]["near_draw"]):
                live[b] = False
        comp.append(torch.tensor(live.copy()))
        tok = torch.where(finished, torch.full_like(tok, eos), tok)
        toks.append(tok)
        finished = finished | (tok == eos)
        if bool(finished.all()):
            break
        nxt = torch.nn.functional.embedding(tok, w[R.LLM_PREFIX + "embed_tokens.weight"])[:, None, :]
    return torch.stack(toks, dim=1), torch.stack(comp, dim=1)
