"""The attention checker has power (no GPU): a plain-torch emulation of the bf16 kernels' rounding points passes
tests/attn_check.py at the bf16 constants, and each of the usual ways these kernels go wrong, applied to that emulation, is
flagged by at least 4x the constant.  `pytest -s` prints which of them whole-tensor rel-L2 at the GPU tests' tolerance
(1e-2 for out, 2e-2 for gradients) would have missed.  The last section does the same for mm_attn_decode: an emulation of the
split-K arithmetic on the GPU tests' own cases, nine planted mistakes, each flagged by the bound at >= 4x c or by an exact family."""
import functools
import math

import pytest
import torch

from tests import attn_check as AC
from tests import test_attention_contract_gpu as GPU          # its case lists; nothing in it runs without a GPU
from tests.kernel_check import check_bits

BF = torch.bfloat16
LN2 = math.log(2.0)
BKV = 64


def bf(x):
    return x.to(BF).float()


def emulate_fwd(q, k, v, mask, causal, scale, mut=None, row=None):
    """attn_fwd128q / attn_fwd_kernel arithmetic: 64-key tiles, online softmax in fp32 with base-2 exponentials, l summed from
    the fp32 p, P rounded to bf16 before P.V, out = bf16(O / l), lse = (m + log2 l) ln 2.  `mut` names a deliberate mistake."""
    B, Sq, Hq, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    kvh = torch.arange(Hq) // G
    if mut == "wrong_kv_head":
        kvh[row[1]] = (kvh[row[1]] + 1) % Hkv
    qf = q.float().permute(0, 2, 1, 3)                                     # [B, Hq, Sq, D]
    kf = k.float().permute(0, 2, 1, 3)[:, kvh]
    vf = v.float().permute(0, 2, 1, 3)[:, kvh]
    al = AC.visible(mask, causal, B, Sq, Skv, "cpu")[:, None].expand(B, Hq, Sq, Skv).clone()
    if mut == "drop_diag":                                                # row: (b, h, i)
        b, h, i = row
        al[b, h, i, i + Skv - Sq] = False
    elif mut == "one_past_diag":
        b, h, i = row
        al[b, h, i, i + Skv - Sq + 1] = True
    elif mut == "skip_tile":                                              # row: (b, h, q256 block, 64-key tile)
        b, h, qb, t = row
        al[b, h, qb * 256:(qb + 1) * 256, t * BKV:(t + 1) * BKV] = False
    elif mut == "drop_last_partial":
        t = (Skv - 1) // BKV
        al[..., t * BKV:] = False
    elif mut == "masked_key_visible":                                     # row: (b, key)
        b, j = row
        al[b, :, :, j] = AC.visible(None, causal, B, Sq, Skv, "cpu")[b, :, j][None]
    sc = scale * AC.LOG2E
    m = torch.full((B, Hq, Sq), -math.inf)
    lsum = torch.zeros(B, Hq, Sq)
    o = torch.zeros(B, Hq, Sq, D)
    for t0 in range(0, Skv, BKV):
        s = qf @ kf[:, :, t0:t0 + BKV].transpose(2, 3)
        s = s.masked_fill(~al[..., t0:t0 + BKV], -math.inf)
        m_new = torch.maximum(m, s.amax(-1) * sc)
        m_safe = torch.where(m_new == -math.inf, torch.zeros_like(m_new), m_new)
        alpha = torch.exp2(m - m_safe)
        p = torch.exp2(s * sc - m_safe[..., None])
        lsum = lsum * alpha + p.sum(-1)
        a_o = alpha.clone()
        if mut == "no_rescale" and t0 > 0:                               # this row keeps O when its max moves
            b, h, i = row
            a_o[b, h, i] = 1.0
        o = o * a_o[..., None] + bf(p) @ vf[:, :, t0:t0 + BKV]
        m = m_new
    inv = torch.where(lsum > 0, 1.0 / torch.where(lsum > 0, lsum, torch.ones_like(lsum)), torch.zeros_like(lsum))
    out = (o * inv[..., None]).to(BF).permute(0, 2, 1, 3).contiguous()
    lse = torch.where(lsum > 0, (m + torch.log2(torch.where(lsum > 0, lsum, torch.ones_like(lsum)))) * LN2,
                      torch.full_like(lsum, math.inf))
    if mut == "copy_neighbour":
        b, h, i = row
        out[b, i, h] = out[b, i + 1, h]
    return out, lse


def emulate_bwd(q, k, v, out, dout, lse, mask, causal, scale, mut=None, row=None):
    """attn_bwd_dq128p / attn_bwd_dkv128_pairp arithmetic: delta from the bf16 out, p = exp2(S*scale*log2e - lse*log2e) in fp32,
    dS = bf16(p (dP - delta) scale), dV = bf16(P)^T.dO, dK = dS^T.Q summed over the group's heads, dQ = dS.K, all rounded to bf16."""
    B, Sq, Hq, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    kvh = torch.arange(Hq) // G
    lse = lse.clone()
    if mut == "lse_ln2":
        b, h, i = row
        lse[b, h, i] += LN2
    qf = q.float().permute(0, 2, 1, 3)
    kf = k.float().permute(0, 2, 1, 3)[:, kvh]
    vf = v.float().permute(0, 2, 1, 3)[:, kvh]
    dof = dout.float().permute(0, 2, 1, 3)
    delta = (out.float() * dout.float()).sum(-1).permute(0, 2, 1)          # [B, Hq, Sq]
    al = AC.visible(mask, causal, B, Sq, Skv, "cpu")[:, None]
    s = qf @ kf.transpose(2, 3)
    p = torch.exp2(s * (scale * AC.LOG2E) - (lse * AC.LOG2E)[..., None])
    p = torch.where(al, p, torch.zeros_like(p))
    dp = dof @ vf.transpose(2, 3)
    ds = bf(p * (dp - delta[..., None]) * scale)
    pb = bf(p)
    dq = (ds @ kf).permute(0, 2, 1, 3).to(BF)
    dk_h = ds.transpose(2, 3) @ qf                                          # [B, Hq, Skv, D]
    dv_h = pb.transpose(2, 3) @ dof
    if mut == "dkv_lose_head":                                            # row: (b, hq, 128-key block)
        b, h, kb = row
        dk_h[b, h, kb * 128:(kb + 1) * 128] = 0
        dv_h[b, h, kb * 128:(kb + 1) * 128] = 0
    dk = dk_h.reshape(B, Hkv, G, Skv, D).sum(2).permute(0, 2, 1, 3).to(BF)
    dv = dv_h.reshape(B, Hkv, G, Skv, D).sum(2).permute(0, 2, 1, 3).to(BF)
    if mut == "swap_dq_tiles":                                            # row: (b, h, 32-row tile): swapped with the next
        b, h, t = row
        a0, a1 = dq[b, t * 32:(t + 1) * 32, h].clone(), dq[b, (t + 1) * 32:(t + 2) * 32, h].clone()
        dq[b, t * 32:(t + 1) * 32, h], dq[b, (t + 1) * 32:(t + 2) * 32, h] = a1, a0
    return dq, dk, dv


def make_inputs(B, Sq, Skv, Hq, Hkv, D, seed, mag="randn"):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Sq, Hq, D, generator=g)
    k = torch.randn(B, Skv, Hkv, D, generator=g)
    v = torch.randn(B, Skv, Hkv, D, generator=g)
    do = torch.randn(B, Sq, Hq, D, generator=g)
    if mag == "big":                                                      # scores up to ~ +-60 after scaling
        q, k = q * 2.8, k * 2.8
    elif mag == "rising":                                                 # the running max moves in every tile
        q[..., 0] = 4.0
        k[..., 0] = torch.linspace(-1.0, 1.0, Skv)[None, :, None] * (40.0 / (4.0 * D ** -0.5))
    return q.to(BF), k.to(BF), v.to(BF), do.to(BF)


def holes_mask(B, Skv):
    m = torch.ones(B, Skv, dtype=torch.long)
    m[0, 70:73] = 0                        # a hole inside one 64-key tile
    if Skv > 200:
        m[0, 128:192] = 0                  # a fully masked 64-key tile between visible ones
    if B > 1:
        m[1, :Skv // 3] = 0                # left padding
    return m


def run(case, mut_f=None, mut_b=None, row=None):
    B, Sq, Skv, Hq, Hkv, D, causal, masked, mag = case
    q, k, v, do = make_inputs(B, Sq, Skv, Hq, Hkv, D, 7 + Sq + D, mag)
    mask = holes_mask(B, Skv) if masked else None
    scale = D ** -0.5
    ref = AC.reference(q, k, v, do, mask, causal, scale)
    out, lse = emulate_fwd(q, k, v, mask, causal, scale, mut_f, row)
    if mut_f is not None:   # the backward reads the forward's (correct) out and lse; a forward mistake is checked on out
        out_b, lse_b = emulate_fwd(q, k, v, mask, causal, scale)
    else:
        out_b, lse_b = out, lse
    dq, dk, dv = emulate_bwd(q, k, v, out_b, do, lse_b, mask, causal, scale, mut_b, row)
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv), ref, mask


def ratios(res, ref):
    big = {n: math.inf for n in ("out", "lse", "dq", "dk", "dv")}
    return AC.check_all(res, ref, BF, None, c=big)


CLEAN = [
    # B, Sq, Skv, Hq, Hkv, D, causal, masked, magnitude
    (2, 130, 130, 4, 2, 64, True, True, "randn"),
    (1, 200, 300, 3, 1, 128, True, False, "randn"),
    (2, 97, 257, 2, 2, 128, False, True, "big"),
    (1, 70, 70, 4, 1, 128, True, False, "rising"),
    (1, 100, 60, 2, 1, 64, True, False, "randn"),        # Sq > Skv: the first 40 rows see no key
    (2, 65, 65, 7, 1, 128, True, True, "big"),
]


@pytest.mark.parametrize("case", CLEAN)
def test_emulation_passes(case):
    res, ref, _ = run(case)
    D = case[5]
    c = AC.C["bf16-d128" if D == 128 else "bf16-d64"]
    AC.check_all(res, ref, BF, "bf16-d128" if D == 128 else "bf16-d64", c=c)
    AC.check_contract(res, ref)


# name, case, forward mutation, backward mutation, row argument
MUTATIONS = [
    ("one row loses its diagonal key", (1, 160, 160, 2, 1, 128, True, False, "randn"), "drop_diag", None, (0, 1, 40)),
    ("one row sees the key one past its diagonal", (1, 160, 160, 2, 1, 128, True, False, "randn"), "one_past_diag", None, (0, 0, 90)),
    ("one 64-key tile skipped for one 256-row block", (1, 300, 300, 2, 1, 128, False, False, "randn"), "skip_tile", None, (0, 1, 1, 2)),
    ("last partial key tile dropped", (1, 64, 300, 2, 1, 128, False, False, "randn"), "drop_last_partial", None, None),
    ("one query head reads the wrong KV head", (1, 100, 100, 4, 2, 128, True, False, "randn"), "wrong_kv_head", None, (0, 1, 0)),
    ("one row copied from its neighbour", (1, 200, 200, 2, 1, 64, True, False, "randn"), "copy_neighbour", None, (0, 1, 150)),
    ("one row misses the rescale when its max moves", (1, 200, 200, 2, 1, 128, True, False, "rising"), "no_rescale", None, (0, 0, 180)),
    ("lse off by ln 2 on one row (backward)", (1, 160, 160, 2, 1, 128, True, False, "randn"), None, "lse_ln2", (0, 1, 120)),
    ("one masked key treated as visible", (2, 130, 260, 2, 1, 128, False, True, "randn"), "masked_key_visible", None, (0, 71)),
    ("dk/dv of one 128-key block lose one query head (odd G)", (1, 65, 257, 7, 1, 128, True, False, "randn"), None, "dkv_lose_head", (0, 6, 1)),
    ("two 32-row dq tiles swapped", (1, 200, 200, 2, 1, 128, True, False, "randn"), None, "swap_dq_tiles", (0, 1, 3)),
]

TOL_OUT, TOL_GRAD = 1e-2, 2e-2      # the whole-tensor rel-L2 of tests/test_kernels_gpu.py


def _rel(a, b):
    a, b = a.double(), b.double()
    ok = torch.isfinite(b)
    return float((a[ok] - b[ok]).norm() / (b[ok].norm() + 1e-30))


@pytest.mark.parametrize("mutation", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutation_flagged(mutation):
    name, case, mf, mb, row = mutation
    D = case[5]
    path = "bf16-d128" if D == 128 else "bf16-d64"
    res, ref, _ = run(case, mf, mb, row)
    r = ratios(res, ref)
    worst_q, ratio = max(((n, r[n] / AC.C[path][n]) for n in r), key=lambda x: x[1])
    assert ratio >= 4.0, f"{name}: worst err/(c u E) = {ratio:.2f} ({worst_q}), needs >= 4"
    rl2 = {n: _rel(res[n].float(), ref[n]) for n in ("out", "dq", "dk", "dv")}
    missed = rl2["out"] < TOL_OUT and max(rl2["dq"], rl2["dk"], rl2["dv"]) < TOL_GRAD
    print(f"\n  [{name}] flagged by {ratio:.1f}x c on {worst_q}; whole-tensor rel-L2 out {rl2['out']:.2e} "
          f"dq {rl2['dq']:.2e} dk {rl2['dk']:.2e} dv {rl2['dv']:.2e} -> "
          f"{'MISSED by rel-L2' if missed else 'seen by rel-L2'}")


# ---- mm_attn_decode: the split-K arithmetic, on the shapes of the GPU tests --------------------------------------------------------
DECODE_C = AC.C["bf16-decode-valu"]["out"]


def emulate_decode(q, k, v, mask, scale, nsplit, mut=None):
    """attn_decode_partial_kernel + the merge in plain torch: per slice an online softmax in fp32 with base-2 exponentials (here
    the slice's max taken at once), a record (m, l, o) per (sequence, head, slice) -- (-inf, 0, 0) for a slice with no visible key
    --, the merge in slice order with the max rescale, ONE rounding to bf16; 0 where no key is visible.  `mut` names a deliberate
    mistake; a mistake inside a slice or in the merge is planted in slice 1 (slice 0 where there is only one) of ONE row, the
    last head of the last sequence."""
    B, Hq, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    chunk = AC.decode_chunk(Skv, nsplit)
    st = 1 if chunk < Skv else 0
    kvh, qsrc = torch.arange(Hq) // G, torch.arange(Hq)
    if mut == "wrong_kv_head":
        kvh[-1] = (kvh[-1] + 1) % Hkv
    if mut == "next_query" and G > 1:
        qsrc[0] = 1
    qf = q.float()[:, qsrc] * (scale * AC.LOG2E)
    kf = k.float().permute(0, 2, 1, 3)[:, kvh]                               # [B, Hq, Skv, D]
    vf = v.float().permute(0, 2, 1, 3)[:, kvh]
    vis = torch.ones(B, Skv, dtype=torch.bool) if mask is None else mask != 0
    s = torch.einsum("bhd,bhkd->bhk", qf, kf)
    ms, ls, os_ = [], [], []
    for sl in range(nsplit):
        k0, k1 = sl * chunk, min(Skv, (sl + 1) * chunk)
        if k0 >= k1:                                                         # a slice with no key at all
            empty_l = 1.0 if mut == "empty_l_one" else 0.0
            ms.append(torch.full((B, Hq), 0.0 if mut == "empty_l_one" else -math.inf))
            ls.append(torch.full((B, Hq), empty_l))
            os_.append(torch.zeros(B, Hq, D))
            continue
        al = vis[:, k0:k1].clone()
        mult = torch.ones(k1 - k0)
        if sl == st:
            if mut == "drop_last":
                al[:, -1] = False
            elif mut == "first_twice":
                mult[0] = 2.0
            elif mut == "mask_ignored":
                al[:] = True
        ss = s[:, :, k0:k1].masked_fill(~al[:, None], -math.inf)
        m = ss.amax(-1)
        p = torch.exp2(ss - torch.where(m == -math.inf, torch.zeros_like(m), m)[..., None]) * mult
        ms.append(m)
        ls.append(p.sum(-1))
        os_.append(torch.einsum("bhk,bhkd->bhd", p, vf[:, :, k0:k1]))
    if mut == "skip_slice" and len(ms) > 1:
        del ms[st], ls[st], os_[st]
    M, L, O = torch.stack(ms), torch.stack(ls), torch.stack(os_)
    mn = M.amax(0)
    al = torch.exp2(M - torch.where(mn == -math.inf, torch.zeros_like(mn), mn))
    if mut == "no_rescale":
        al = torch.ones_like(al)
    lt, ot = (L * al).sum(0), (O * al[..., None]).sum(0)
    out = torch.where(lt[..., None] > 0, ot / torch.where(lt > 0, lt, torch.ones_like(lt))[..., None], torch.zeros_like(ot))
    if mut == "dead_mean":
        dead = ~vis.any(-1)
        out[dead] = vf.mean(2)[dead]
    if mut in SLICE_MUTATIONS:                        # planted in ONE row: the last head of the last sequence
        clean = emulate_decode(q, k, v, mask, scale, nsplit).float()
        clean[B - 1, Hq - 1] = out[B - 1, Hq - 1]
        out = clean
    return out.to(BF)


SLICE_MUTATIONS = ("drop_last", "first_twice", "skip_slice", "no_rescale", "mask_ignored", "empty_l_one")


@functools.lru_cache(maxsize=None)
def decode_problem(i):
    """operands, mask, split count and the fp64 reference of GPU.DECODE_CASES[i], computed once"""
    c = GPU.DECODE_CASES[i]
    ns = AC.decode_nsplit(c)
    mask = AC.decode_mask(c["mask"], c["B"], c["Skv"], ns)
    q, k, v = AC.decode_operands(c, mask)
    return c, ns, mask, q, k, v, AC.decode_reference(q, k, v, mask, c["D"] ** -0.5)


def decode_exact(mut):
    """the exact families on the GPU tests' shapes -> the names of those whose bits the emulation misses"""
    bad = []
    for fam, cases, make in (("one_key", GPU.ONE_KEY_CASES, AC.decode_one_key), ("uniform", GPU.UNIFORM_CASES, None)):
        for c in cases:
            ns = AC.decode_nsplit(c)
            q, k, v, mask, want = make(c, ns) if make else AC.decode_uniform(c)
            got = emulate_decode(q, k, v, mask, c["D"] ** -0.5, ns, mut)
            try:
                check_bits(fam, got, want, zero_sign=False)
            except AssertionError:
                bad.append(f"{fam} {AC.decode_case_id(c)}")
    return bad


def test_decode_case_lists_reach_every_edge():
    cs = GPU.DECODE_CASES
    for D in (64, 128):
        assert {c["Hq"] // c["Hkv"] for c in cs if c["D"] == D} == {1, 2, 4, 7, 8}
        # every length through each kernel: D = 64 is VALU for every G; at D = 128 the G <= 4 cases run MFMA and VALU both
        assert {1, 15, 17, 63, 65, 129, 200, 2051} <= {c["Skv"] for c in cs if c["D"] == D and (D == 64 or c["Hq"] // c["Hkv"] <= 4)}
    assert {c["B"] for c in cs} == {1, 3} and {c["Hkv"] for c in cs} == {1, 2}
    assert {c["mask"] for c in cs} == {None, "leftpad", "holes", "slice", "dead", "single"}
    assert {"lib", "lib8", 1, 3, 8} <= {c["ns"] for c in cs}
    assert any(c["ns"] == 3 and c["Skv"] == 200 for c in cs) and any(c["ns"] == 8 and c["Skv"] == 10 for c in cs)
    assert AC.decode_nsplit(AC.decode_case(1, 2051, 4, 1, 128)) == 33 and AC.decode_nsplit(AC.decode_case(3, 129, 2, 1, 128, ns="lib8")) == 3


def test_decode_emulation_passes():
    worst = 0.0
    for i in range(len(GPU.DECODE_CASES)):
        c, ns, mask, q, k, v, ref = decode_problem(i)
        out = emulate_decode(q, k, v, mask, c["D"] ** -0.5, ns)
        worst = max(worst, AC.check_decode(out, ref, "bf16-decode-emulation", c=DECODE_C))
        assert bool((out[~ref["rows"]] == 0).all())
    assert decode_exact(None) == []
    assert worst < DECODE_C
    print(f"\n  [decode emulation] worst err/(u E) = {worst:.3f} (c = {DECODE_C})")


DECODE_MUTATIONS = [("the last key of a slice dropped", "drop_last"), ("the first key of a slice counted twice", "first_twice"),
                    ("one slice skipped by the merge", "skip_slice"), ("the merge without the max rescale", "no_rescale"),
                    ("the mask ignored inside one slice", "mask_ignored"), ("head g reads head g+1's query", "next_query"),
                    ("the wrong kv head", "wrong_kv_head"), ("a fully masked row returns the mean of V", "dead_mean"),
                    ("an empty slice contributes l = 1", "empty_l_one")]


@pytest.mark.parametrize("mutation", DECODE_MUTATIONS, ids=[m[1] for m in DECODE_MUTATIONS])
def test_decode_mutation_flagged(mutation):
    name, mut = mutation
    best, where, hit, missed = 0.0, None, 0, []
    for i in range(len(GPU.DECODE_CASES)):
        c, ns, mask, q, k, v, ref = decode_problem(i)
        out = emulate_decode(q, k, v, mask, c["D"] ** -0.5, ns, mut)
        if torch.equal(out, emulate_decode(q, k, v, mask, c["D"] ** -0.5, ns)):
            continue                                                         # the mistake has no effect at this shape
        hit += 1
        try:
            ratio = AC.check_decode(out, ref, None, c=math.inf) / DECODE_C
        except AssertionError:                                               # a non-finite value, or != 0 where E = 0
            ratio = math.inf
        if _rel(out.float(), ref["out"]) < TOL_OUT:
            missed.append(f"{AC.decode_case_id(c)} (bound: {ratio:.1f}x c)")
        if ratio > best:
            best, where = ratio, AC.decode_case_id(c)
    exact = decode_exact(mut)
    assert best >= 4.0 or exact, f"{name}: worst err/(c u E) = {best:.2f} and no exact family flags it"
    print(f"\n  [decode: {name}] changes the output of {hit} GPU cases; bound: {best:.1f}x c at {where}; exact-family cases that "
          f"flag it: {len(exact)}; whole-tensor rel-L2 at {TOL_OUT} MISSES it in {len(missed)} of the {hit}: {missed}")
