"""Attention checker: an fp64 reference with per-element error scales, the output contract, and guarded launches.

`reference` runs in float64 on the device of its operands, on the SAME bf16- or fp32-rounded q/k/v/dout the kernels read.
Besides out, lse (natural log), dq, dk and dv it returns the error scale E of every element for the rule of tests/kernel_check.py
(c per path: `C` below).  E = 0, where the result must be exact: rows with no visible key (out = 0, lse = +inf, dq = 0) and masked
keys (dk = dv = 0).

The rounding points of the bf16 kernels (mm_attn.hip) and the term of E that covers each:
  forward   scores S = Q.K^T in fp32 (exact bf16 products), p = exp2(S*scale*log2e - m) in fp32, l summed from the fp32 p,
            P rounded to bf16 before O += P.V, out = bf16(O / l)                      -> E_o  = P.|V|   (P rounding + out rounding)
  backward  delta = rowsum(out * dO) from the bf16 `out`                           -> |o|.|dO| term of E_dS (carried as E_o.|dO|)
            p = exp2(S*scale*log2e - lse*log2e), dP = dO.V^T in fp32
            dV += bf16(P)^T.dO                                                   -> E_dv = P^T.|dO|
            dS = bf16(P * (dP - delta) * scale)                                  -> E_dS = P o (|dP| + |delta| + E_o.|dO| row sums)
            dQ = dS.K, dK = dS^T.Q (fp32 accumulation), every output rounded to bf16 -> E_dq = scale E_dS.|K|, E_dk = scale E_dS^T.|Q|
The fp32 kernels have no bf16 rounding point, and their largest error is the fp32 score itself (a D-term dot product, and the
exponent argument S*scale - lse): each P carries a relative error of ~u32 * A with A = sqrt(D) * scale * |Q|.|K|^T + |lse|.
That enters every scale as P -> P o (1 + kappa * A) (plus kappa * |o| * rowsum(P o A) for out and kappa * sqrt(D) * P o |dO|.|V|^T
for dP), with kappa = u32 / u: 1 for fp32, 2^-16 for bf16 (negligible there).  lse is fp32 in both paths and is checked with
u32 against E_lse = |lse| + rowsum(P o A) + sqrt(visible keys) (the fp32 sum of l).

The bound is a worst-case (sum of |terms|) bound: it is rigorous, and so it loses power as 1/sqrt(n) on long rows -- a
single-key error in a row of n keys moves out by ~1/n of a value while E_o stays ~mean|v|.  tests/test_attn_check_cpu.py shows
at which sizes the usual kernel mistakes are flagged."""
import functools
import math

import torch

from tests.kernel_check import U, U32, Guarded, RatioLog, check_bound, coords, dt, ptr, verify_guards  # noqa: F401

LOG2E = 1.4426950408889634

# c per launch path and quantity: the smallest power of two >= 2x the worst err / (u E) measured on the MI355X over the
# cases of tests/test_attention_contract_gpu.py (the PR description lists the measured ratios)
C = {
    "bf16-d128": {"out": 4.0, "lse": 1.0, "dq": 1.0, "dk": 1.0, "dv": 4.0},        # measured 1.71, 0.30, 0.45, 0.49, 1.85
    # attn_fwd128p_kernel, one case (test_attention_long_kv): measured 0.013, 0.054, 0.002, 0.23, 1.17; its siblings' constants
    "bf16-d128-long": {"out": 4.0, "lse": 1.0, "dq": 1.0, "dk": 1.0, "dv": 4.0},
    "bf16-d64": {"out": 4.0, "lse": 1.0, "dq": 1.0, "dk": 2.0, "dv": 4.0},         # measured 1.58, 0.38, 0.43, 0.59, 1.79
    "f32": {"out": 2.0, "lse": 2.0, "dq": 0.25, "dk": 0.25, "dv": 2.0},            # measured 0.59, 0.75, 0.10, 0.09, 0.62
    # mm_attn_decode.  DERIVED, not measured: the decode kernels keep P in fp32, so their one bf16 rounding is out = bf16(o / l)
    # with |o / l| <= P.|V| = E_out, err / (u E) <= 1; the fp32 score, exp2 and accumulation errors sit in E through the kappa
    # terms.  c = 1 (the rounding) x 2 (margin).  The measured ratios are beside each path for the record only.
    "bf16-decode-valu": {"out": 2.0},      # attn_decode_partial_kernel + attn_decode_merge_kernel: measured 0.855
    "bf16-decode-mfma": {"out": 2.0},      # attn_decode_partial128_mfma_kernel + merge: measured 0.855
    "bf16-decode-fused": {"out": 2.0},     # attn_decode_partial_kernel, merged by the last slice (sync): measured 0.855
}

# worst err / (u E) seen per (path, quantity) in this process; MM_ATTN_RATIO_LOG=<file> writes them out at exit
RATIOS = RatioLog("MM_ATTN_RATIO_LOG")


def path_of(dtype, D, Skv):
    if dtype == torch.float32:
        return "f32"
    if D == 64:
        return "bf16-d64"
    return "bf16-d128" if Skv <= 256 * 1024 else "bf16-d128-long"


def visible(key_mask, causal, B, Sq, Skv, device):
    """[B, Sq, Skv] bool: key j is visible to query i (causal: j <= i + Skv - Sq, the ABI's alignment; covers Sq > Skv)."""
    allowed = torch.ones(B, Sq, Skv, dtype=torch.bool, device=device)
    if causal:
        allowed &= (torch.arange(Skv, device=device)[None, :] <= torch.arange(Sq, device=device)[:, None] + (Skv - Sq))[None]
    if key_mask is not None:
        allowed &= (key_mask.to(device) != 0)[:, None, :]
    return allowed


def reference(q, k, v, dout, key_mask, causal, scale, backward=True):
    """fp64 on q's device.  q/dout [B,Sq,Hq,D], k/v [B,Skv,Hkv,D] (any strides).  Returns a dict with out, lse [B,Hq,Sq],
    dq, dk, dv (fp64, the operands' layouts) and their error scales E_out, E_lse, E_dq, E_dk, E_dv, plus rows [B,Sq]
    (the query has at least one visible key) and keys [B,Skv] (the key is visible to at least one query)."""
    B, Sq, Hq, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    dev = q.device
    kappa = U32 / U[q.dtype]
    rt = math.sqrt(D)
    f64 = dict(dtype=torch.float64, device=dev)
    r = {n: torch.zeros(B, Sq, Hq, D, **f64) for n in ("out", "E_out", "dq", "E_dq")}
    r.update({n: torch.zeros(B, Skv, Hkv, D, **f64) for n in ("dk", "E_dk", "dv", "E_dv")})
    r["lse"] = torch.full((B, Hq, Sq), math.inf, **f64)
    r["E_lse"] = torch.zeros(B, Hq, Sq, **f64)
    allowed = visible(key_mask, causal, B, Sq, Skv, dev)
    r["rows"] = allowed.any(-1)
    r["keys"] = allowed.any(1)
    for b in range(B):
        al = allowed[b]
        nvis = al.sum(-1).double()                                      # [Sq]
        for hkv in range(Hkv):
            hs = slice(hkv * G, (hkv + 1) * G)
            Q = q[b, :, hs].double().permute(1, 0, 2)                   # [G, Sq, D]
            Kt, V = k[b, :, hkv].double(), v[b, :, hkv].double()         # [Skv, D]
            S = (Q @ Kt.t() * scale).masked_fill(~al, -math.inf)
            m = S.amax(-1, keepdim=True) if Skv else torch.full((G, Sq, 1), -math.inf, **f64)
            m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
            e = torch.exp(S - m)
            del S
            lsum = e.sum(-1, keepdim=True)
            P = e / torch.where(lsum > 0, lsum, torch.ones_like(lsum))
            del e
            lse = torch.where(lsum > 0, m + torch.log(lsum), torch.full_like(m, math.inf))
            lse_fin = torch.where(lsum > 0, lse, torch.zeros_like(lse))
            O = P @ V
            PA = P * (rt * scale * (Q.abs() @ Kt.abs().t()) + lse_fin.abs())
            Pw = P + kappa * PA
            PA_sum = PA.sum(-1, keepdim=True)
            del PA
            E_o = Pw @ V.abs() + kappa * O.abs() * PA_sum
            r["out"][b, :, hs] = O.permute(1, 0, 2)
            r["E_out"][b, :, hs] = E_o.permute(1, 0, 2)
            r["lse"][b, hs] = lse[..., 0]
            r["E_lse"][b, hs] = (lse_fin.abs() + PA_sum)[..., 0] + nvis.sqrt()[None]
            if not backward:
                continue
            dO = dout[b, :, hs].double().permute(1, 0, 2)
            dP = dO @ V.t()
            delta = (O * dO).sum(-1, keepdim=True)
            E_delta = (E_o * dO.abs()).sum(-1, keepdim=True)
            dS = P * (dP - delta)
            E_dS = Pw * (dP.abs() + delta.abs()) + P * E_delta + kappa * rt * P * (dO.abs() @ V.abs().t())
            del dP
            r["dq"][b, :, hs] = (scale * dS @ Kt).permute(1, 0, 2)
            r["E_dq"][b, :, hs] = (scale * E_dS @ Kt.abs()).permute(1, 0, 2)
            r["dk"][b, :, hkv] = scale * (dS.transpose(1, 2) @ Q).sum(0)
            r["E_dk"][b, :, hkv] = scale * (E_dS.transpose(1, 2) @ Q.abs()).sum(0)
            r["dv"][b, :, hkv] = (P.transpose(1, 2) @ dO).sum(0)
            r["E_dv"][b, :, hkv] = (Pw.transpose(1, 2) @ dO.abs()).sum(0)
            del dS, E_dS, P, Pw
    return r


def _where(kind, idx, shape):
    """Human-readable location of flat index idx in a tensor of `kind` ('q': [B,Sq,Hq,D], 'k': [B,Skv,Hkv,D], 'lse': [B,Hq,Sq])
    with its tile coordinates (32- and 256-row query blocks, 64- and 128-key blocks)."""
    if kind == "lse":
        b, h, row = coords(idx, shape)
        return f"(b={b}, row={row}, head={h}) [q32 tile {row // 32}, q256 block {row // 256}]"
    b, row, h, d = coords(idx, shape)
    if kind == "q":
        return f"(b={b}, row={row}, head={h}, d={d}) [q32 tile {row // 32}, q256 block {row // 256}]"
    return f"(b={b}, key={row}, kvhead={h}, d={d}) [k64 tile {row // 64}, k128 block {row // 128}]"


def check(name, got, ref, E, c, u, kind, path=None):
    """The rule on one quantity (lse: exact also where ref = +inf, a row with no visible key); recorded in RATIOS[(path, name)];
    a failure names the element's tiles."""
    return check_bound(name, got, ref, E, c, u, key=path and (path, name), log=RATIOS, where=functools.partial(_where, kind),
                       exact=torch.isinf(ref) if kind == "lse" else None)


def check_all(res, ref, dtype, path, c=None, backward=True):
    """Every quantity of `res` (dict with out, lse and, for backward, dq, dk, dv) against `ref`; returns {name: worst ratio}."""
    c = c or C[path]
    u = U[dtype]
    out = {"out": check("out", res["out"], ref["out"], ref["E_out"], c["out"], u, "q", path),
           "lse": check("lse", res["lse"], ref["lse"], ref["E_lse"], c["lse"], U32, "lse", path)}
    if backward:
        out["dq"] = check("dq", res["dq"], ref["dq"], ref["E_dq"], c["dq"], u, "q", path)
        out["dk"] = check("dk", res["dk"], ref["dk"], ref["E_dk"], c["dk"], u, "k", path)
        out["dv"] = check("dv", res["dv"], ref["dv"], ref["E_dv"], c["dv"], u, "k", path)
    return out


def check_contract(res, ref, backward=True):
    """The output contract: rows with no visible key give out == 0, lse == +inf, dq == 0 exactly; keys no query
    sees (masked) give dk == dv == 0 exactly; every output is finite (lse: finite or +inf)."""
    rows, keys = ref["rows"].to(res["out"].device), ref["keys"].to(res["out"].device)
    out, lse = res["out"], res["lse"]
    dead = ~rows                                                        # [B, Sq]
    assert bool(torch.isfinite(out).all()), "out has non-finite values"
    assert bool((out[dead] == 0).all()), "out != 0 on a row with no visible key"
    assert bool(torch.isinf(lse.transpose(1, 2)[dead]).all()) and bool((lse.transpose(1, 2)[dead] > 0).all()), \
        "lse != +inf on a row with no visible key"
    assert bool(torch.isfinite(lse.transpose(1, 2)[rows]).all()), "lse not finite on a row with visible keys"
    if backward:
        dq, dk, dv = res["dq"], res["dk"], res["dv"]
        for n, t in (("dq", dq), ("dk", dk), ("dv", dv)):
            assert bool(torch.isfinite(t).all()), f"{n} has non-finite values"
        assert bool((dq[dead] == 0).all()), "dq != 0 on a row with no visible key"
        assert bool((dk[~keys] == 0).all()) and bool((dv[~keys] == 0).all()), "dk/dv != 0 on a key no query sees"


# ---- guarded launches through the C ABI --------------------------------------------------------------------------------
def grad_views(views, zero=()):
    """Gradient buffers with the SAME strides and offsets as the operand views (the ABI's rule), in guarded storages that mirror
    the operands' storages: views that share a storage (the fused qkv buffer) share one guarded storage, so the columns
    between the q, k and v sections and the rows past a prefix view are guards.  Views named in `zero` are zero-filled."""
    stores, out = {}, []
    for i, x in enumerate(views):
        key = x.untyped_storage().data_ptr()
        if key not in stores:
            stores[key] = Guarded(x.untyped_storage().nbytes() // x.element_size(), x.dtype, x.device)
        g = stores[key].view(x.shape, x.stride(), x.storage_offset())
        if i in zero:
            g.zero_()
        out.append(g)
    return out, list(stores.values())


def _s3(t):
    return t.stride(0), t.stride(1), t.stride(2)


def run_fwd(q, k, v, key_mask, causal, scale, stream=None):
    """mm_attn_fwd with out / lse inside guarded storages; returns (out, lse, [guards])."""
    from multimeditron_amd._lib import call
    B, Sq, Hq, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    go = Guarded(B * Sq * Hq * D, q.dtype, q.device)
    gl = Guarded(B * Hq * Sq, torch.float32, q.device)
    out = go.view((B, Sq, Hq, D), (Sq * Hq * D, Hq * D, D, 1))
    lse = gl.view((B, Hq, Sq), (Hq * Sq, Sq, 1))
    st = stream if stream is not None else torch.cuda.current_stream()
    call("mm_attn_fwd", dt(q.dtype), ptr(q), ptr(k), ptr(v), B, Sq, Skv, Hq, Hkv, D, *_s3(q), *_s3(k), *_s3(v), ptr(key_mask),
         int(causal), float(scale), ptr(out), ptr(lse), st.cuda_stream)
    return out, lse, [("out", go), ("lse", gl)]


def run_bwd(q, k, v, out, dout, lse, key_mask, causal, scale, stream=None):
    """mm_attn_bwd with dq/dk/dv as guarded views mirroring q/k/v (fp32: dk/dv zero-filled, as the ABI requires);
    returns (dq, dk, dv, [guards])."""
    from multimeditron_amd._lib import call
    B, Sq, Hq, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    (dq, dk, dv), stores = grad_views([q, k, v], zero=(1, 2) if q.dtype == torch.float32 else ())
    delta = torch.empty(B * Hq * Sq, dtype=torch.float32, device=q.device)
    st = stream if stream is not None else torch.cuda.current_stream()
    call("mm_attn_bwd", dt(q.dtype), ptr(q), ptr(k), ptr(v), ptr(out), ptr(dout), ptr(lse), B, Sq, Skv, Hq, Hkv, D, *_s3(q),
         *_s3(k), *_s3(v), ptr(key_mask), int(causal), float(scale), ptr(dq), ptr(dk), ptr(dv), ptr(delta), st.cuda_stream)
    return dq, dk, dv, [(f"dq/dk/dv storage {i}", g) for i, g in enumerate(stores)]


# ---- mm_attn_decode: one query token over a KV cache, split over slices of the keys --------------------------------------------
# The reference is `reference(..., backward=False)` with Sq = 1.  What is below: the launch path names, the split count mirrored
# from mm_attn_decode_splits, the problems of tests/test_attention_contract_gpu.py (shared with the emulation of
# tests/test_attn_check_cpu.py) and the guarded launch.
BF16 = torch.bfloat16
SYNC_SPARE = 5                       # counters behind B * Hkv that no launch may touch
DECODE_WGS = 768                     # g_attn_decode_wgs, the library's default for option attn_decode_wgs


def decode_path(D, G, fused=False, mfma=True):
    """the kernel mm_attn_decode launches: MFMA scores for D = 128, G <= 4 in the two-launch form unless attn_decode_mfma = 0"""
    if fused:
        return "bf16-decode-fused"
    return "bf16-decode-mfma" if mfma and D == 128 and G <= 4 else "bf16-decode-valu"


def decode_splits(B, Hkv, Skv, wgs=DECODE_WGS):
    """mm_attn_decode_splits: ceil(wgs / (B Hkv)) slices, at least 64 keys each, at least one."""
    return max(1, min(-(-wgs // (B * Hkv)), -(-Skv // 64)))


def decode_chunk(Skv, nsplit):
    """keys per slice: slice s holds [s chunk, min(Skv, (s + 1) chunk)), which is empty once s chunk >= Skv"""
    return -(-Skv // nsplit)


def decode_case(B, Skv, Hq, Hkv, D, mask=None, ns="lib"):
    """ns: "lib" / "lib8" = the library's split count under attn_decode_wgs = 768 / 8, or an explicit nsplit"""
    return dict(B=B, Skv=Skv, Hq=Hq, Hkv=Hkv, D=D, mask=mask, ns=ns)


def decode_case_id(c):
    return f"B{c['B']}-k{c['Skv']}-h{c['Hq']}x{c['Hkv']}-d{c['D']}-{c['mask'] or 'nomask'}-ns{c['ns']}"


def decode_nsplit(c):
    if c["ns"] in ("lib", "lib8"):
        return decode_splits(c["B"], c["Hkv"], c["Skv"], 8 if c["ns"] == "lib8" else DECODE_WGS)
    return int(c["ns"])


def decode_mask(kind, B, Skv, nsplit):
    """[B, Skv] int64 or None.  leftpad: the first third (one key less per sequence); holes: every fifth key and a run;
    slice: exactly the keys of one slice (a different one per sequence); dead: every key of sequence 0; single: one visible key."""
    if kind is None:
        return None
    m = torch.ones(B, Skv, dtype=torch.long)
    chunk = decode_chunk(Skv, nsplit)
    for b in range(B):
        if kind == "leftpad":
            m[b, :max(0, Skv // 3 - b)] = 0
        elif kind == "holes":
            m[b, 3 + b::5] = 0
            m[b, 20:40 + b] = 0
        elif kind == "slice":
            assert nsplit > 1, "with one slice this is the dead row"
            s = (b + 1) % min(nsplit, -(-Skv // chunk))
            m[b, s * chunk:(s + 1) * chunk] = 0
        elif kind == "dead":
            if b == 0:
                m[b] = 0
        elif kind == "single":
            m[b] = 0
            m[b, (Skv - 1, 0, Skv // 2)[b % 3]] = 1
        else:
            raise ValueError(kind)
    return m


def decode_operands(c, mask, seed=1):
    """q [B, Hq, D], k / v [B, Skv, Hkv, D] in bf16 (CPU).  Masked keys hold finite values about 1e3 times the visible ones: a
    weight that leaks is loud, and 0 * v stays 0."""
    B, Skv, Hq, Hkv, D = c["B"], c["Skv"], c["Hq"], c["Hkv"], c["D"]
    g = torch.Generator().manual_seed(seed + 13 * Skv + D + Hq)
    q = torch.randn(B, Hq, D, generator=g)
    k = torch.randn(B, Skv, Hkv, D, generator=g)
    v = torch.randn(B, Skv, Hkv, D, generator=g)
    if mask is not None:
        big = torch.where(mask == 0, 1000.0, 1.0)[:, :, None, None]
        k, v = k * big, v * big
    return q.to(BF16), k.to(BF16), v.to(BF16)


def decode_one_key(c, nsplit, seed=2):
    """The exact family `one_key`: one visible key per sequence -- the first key of a slice, the last key of a slice, the key
    Skv - 1, in turn -- so p = exp2(0) = 1 and l = 1: every head of a group returns that key's V row bit for bit.
    -> (q, k, v, mask, want [B, Hq, D])"""
    B, Skv, Hq, Hkv = c["B"], c["Skv"], c["Hq"], c["Hkv"]
    chunk = decode_chunk(Skv, nsplit)
    first = chunk if chunk < Skv else 0
    m = torch.zeros(B, Skv, dtype=torch.long)
    keys = [(first, chunk - 1, Skv - 1)[b % 3] for b in range(B)]
    for b, j in enumerate(keys):
        m[b, j] = 1
    q, k, v = decode_operands(c, m, seed)
    want = torch.stack([v[b, j] for b, j in enumerate(keys)]).repeat_interleave(Hq // Hkv, dim=1)
    return q, k, v, m, want


def decode_uniform(c, nvis=128, seed=3):
    """The exact family `uniform`: q = 0, V small integers in [-2, 2], nvis >> b visible keys in sequence b (powers of two, spread
    evenly over the keys and so over the slices).  Every p is exactly 1, every partial sum is an integer of at most 2 nvis, and
    o / l is exact in bf16: one dropped, doubled or leaked key changes bits.  -> (q, k, v, mask, want [B, Hq, D])"""
    B, Skv, Hq, Hkv, D = c["B"], c["Skv"], c["Hq"], c["Hkv"], c["D"]
    assert nvis <= 128 and nvis & (nvis - 1) == 0 and nvis <= Skv
    g = torch.Generator().manual_seed(seed + Skv)
    m = torch.zeros(B, Skv, dtype=torch.long)
    for b in range(B):
        n = max(1, nvis >> b)
        m[b, (torch.arange(n) * Skv) // n + (b if (n - 1) * Skv // n + b < Skv else 0)] = 1
    q = torch.zeros(B, Hq, D)
    k = torch.randn(B, Skv, Hkv, D, generator=g) * torch.where(m == 0, 1000.0, 1.0)[:, :, None, None]
    v = torch.randint(-2, 3, (B, Skv, Hkv, D), generator=g).double()
    ref = (v * m[:, :, None, None]).sum(1) / m.sum(1)[:, None, None].double()                 # [B, Hkv, D]
    want = ref.float().to(BF16)
    assert bool((want.double() == ref).all()), "uniform family: o / l is not exact in bf16"
    return q.to(BF16), k.to(BF16), v.to(BF16), m, want.repeat_interleave(Hq // Hkv, dim=1)


def decode_place(q, k, v, device="cuda"):
    """The operands as generate() passes them: q a strided view into a fused [B, (Hq + 2 Hkv) D] projection row, k / v prefix
    views [:, :Skv] of a longer cache.  The rest of the row and the cache rows from Skv on hold the sentinel NaN, so a read
    past Skv that reaches the result shows as a non-finite output."""
    from tests.kernel_check import sentinel_fill
    B, Hq, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    row = sentinel_fill(torch.empty(B, (Hq + 2 * Hkv) * D, dtype=q.dtype))
    row[:, :Hq * D] = q.reshape(B, Hq * D)
    kc = sentinel_fill(torch.empty(B, Skv + 11, Hkv, D, dtype=q.dtype))
    vc = sentinel_fill(torch.empty(B, Skv + 11, Hkv, D, dtype=q.dtype))
    kc[:, :Skv], vc[:, :Skv] = k, v
    row, kc, vc = row.to(device), kc.to(device), vc.to(device)
    return row[:, :Hq * D].view(B, Hq, D), kc[:, :Skv], vc[:, :Skv]


def decode_reference(q, k, v, key_mask, scale):
    """fp64 out [B, Hq, D] with its error scale, and rows [B] (the sequence has a visible key; elsewhere E = 0 and out == 0)."""
    r = reference(q[:, None], k, v, None, key_mask, False, scale, backward=False)
    return {"out": r["out"][:, 0], "E_out": r["E_out"][:, 0], "rows": r["rows"][:, 0]}


def _where_decode(idx, shape):
    b, h, d = coords(idx, shape)
    return f"(b={b}, head={h}, d={d})"


def check_decode(out, ref, path, c=None):
    """The rule on a decode output; recorded in RATIOS[(path, "out")]."""
    return check_bound("out", out, ref["out"], ref["E_out"], C[path]["out"] if c is None else c, U[BF16],
                       key=path and (path, "out"), log=RATIOS, where=_where_decode)


def decode_args(q, k, v, key_mask, scale, out, ws, nsplit, sync):
    """mm_attn_decode's arguments up to the stream"""
    B, Hq, D = q.shape
    return (dt(q.dtype), ptr(q), ptr(k), ptr(v), B, k.shape[1], Hq, k.shape[2], D, q.stride(0), q.stride(1), *_s3(k), *_s3(v),
            ptr(key_mask), float(scale), ptr(out), ptr(ws), nsplit, ptr(sync))


def decode_buffers(B, Hq, D, nsplit, device):
    """out [B, Hq, D] and the fp32 workspace [B Hq nsplit (D + 2)] in guarded storages -> (out, ws, [guards]); the workspace is
    verified with require_written: every slice writes its record, an empty one included."""
    go = Guarded(B * Hq * D, BF16, device)
    gw = Guarded(B * Hq * nsplit * (D + 2), torch.float32, device)
    return (go.view((B, Hq, D), (Hq * D, D, 1)), gw.view((B * Hq * nsplit * (D + 2),), (1,)),
            [("out", go), ("workspace", gw, True)])


def run_decode(q, k, v, key_mask, scale, nsplit=None, fused=False, sync=None):
    """mm_attn_decode with out and the workspace inside guarded storages.  nsplit=None takes mm_attn_decode_splits.  fused: the
    single-launch form on `sync`, or on a fresh zeroed tensor with SYNC_SPARE counters behind B * Hkv; after the run the whole
    tensor must still be zero (`decode_sync_clean`).  -> (out, [guards], sync)"""
    from multimeditron_amd._lib import call, lib
    B, Hq, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    ns = lib().mm_attn_decode_splits(B, Hkv, Skv) if nsplit is None else nsplit
    out, ws, guards = decode_buffers(B, Hq, D, ns, q.device)
    if fused and sync is None:
        sync = torch.zeros(B * Hkv + SYNC_SPARE, dtype=torch.int32, device=q.device)
    call("mm_attn_decode", *decode_args(q, k, v, key_mask, scale, out, ws, ns, sync if fused else None),
         torch.cuda.current_stream().cuda_stream)
    return out, guards, sync if fused else None


def decode_sync_clean(sync):
    assert not bool(sync.any()), f"the arrival counters are not left at zero: {sync.tolist()}"
