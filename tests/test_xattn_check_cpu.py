"""The cross-attention checker has power (no GPU).  Plain-torch emulations of the kernels' arithmetic (the header comment of
csrc/mm_xattn.hip: the bf16 kernels' rounding points; the fp32 kernels' sequential fused-multiply-add chains and wave
reductions) pass tests/xattn_check.py at its constants on every case of the GPU contract test at p in {0, 0.1, 0.5, 0.9}; that
run is where the lse and fp32 constants come from (4x its worst ratios over the (case, p) pairs the GPU test runs; `pytest -s`
prints them).  The keep mask rounds the key count to 32, not 16.  And each of the ways these kernels can go wrong, applied to the bf16 emulation, is flagged by more than
2x the constant on the smallest contract case that can show it; `pytest -s` prints which of them the whole-tensor rel-L2 of
tests/test_xattn_gpu.py (2e-2; lse 5e-3) would have passed."""
import functools
import math

import pytest
import torch

from tests import xattn_check as XC

BF, F32 = XC.BF, XC.F32
PS = (0.0, 0.1, 0.5, 0.9)


def bf(x):
    return x.to(BF).float()


def hm(t):
    return t.float().permute(0, 2, 1, 3)                                  # [n, H, N, D]


def back(t, dtype):
    return t.permute(0, 2, 1, 3).to(dtype)                                # [n, N, H, D]


# ---- the bf16 kernels ---------------------------------------------------------------------------------------------------------
def emulate_bf16(q, k, v, do, scale, keep, p, mut=None, arg=None):
    """xattn_fwd_kernel / xattn_bwd_q_kernel / xattn_bwd_kv_kernel: scores in fp32, s*scale, max, exp, sum; pf = bf16(p inv f),
    out = bf16(pf.V), lse = m + log(sum); delta from the bf16 out, p = exp(s*scale - lse), dS = bf16(p (dP f - delta) scale),
    P_drop = bf16(p f); dq, dk, dv rounded to bf16.  `mut` names a deliberate mistake (MUTATIONS below)."""
    Q, Kt, V, dO = hm(q), hm(k), hm(v), hm(do)
    n, H, Nq, D = Q.shape
    Nkv = Kt.shape[2]
    f = keep.float() * XC.inv_keep(p)
    f_fwd = f_bwd = f
    if mut == "mask_row_from_row0":                                       # arg: the flat probability row that reads row 0's flags
        f_fwd = f_bwd = f.clone()
        f_fwd.view(-1, Nkv)[arg] = f.view(-1, Nkv)[0]
    elif mut == "bwd_mask_shifted":
        f_bwd = torch.roll(f, 1, -1)
    elif mut == "bwd_keep_unscaled":
        f_bwd = keep.float()
    elif mut == "mask_kp16":                                              # arg: the mask indexed with KP rounded to 16
        f_fwd = f_bwd = arg.float() * XC.inv_keep(p)
    Ks = Kt
    if mut == "neighbour_k":                                              # arg: the head that reads the next head's K
        Ks = Kt.clone()
        Ks[:, arg] = Kt[:, (arg + 1) % H]

    def forward(m_):
        s = Q @ (Ks if m_ == "neighbour_k" else Kt).transpose(2, 3)
        ss = s * scale
        m = ss.amax(-1, keepdim=True)
        if m_ == "padding_key":                                           # one key past Nkv (zero K row: score 0) is not masked
            m = m.clamp_min(0.0)
        e = torch.exp(ss - m)
        tot = e.sum(-1, keepdim=True)
        if m_ == "padding_key":
            tot = tot + torch.exp(-m)
        inv = 1.0 / tot
        pf = bf(e * inv * f_fwd)
        Vf = V
        if m_ == "last_v_zero":
            Vf = V.clone()
            Vf[:, :, -1] = 0
        o = pf @ Vf
        if m_ == "slice_from_first":                                      # the columns from 64 on computed from V's first columns
            o[..., 64:] = o[..., :D - 64].clone()
        return s, e * inv, bf(o), (m + torch.log(tot))[..., 0]

    s, p_und, out, lse = forward(mut)
    res = {"out": back(out, BF), "lse": lse}
    if mut in ("padding_key", "last_v_zero", "slice_from_first", "neighbour_k"):
        s, p_und, out, lse = forward(None)                                # a forward mistake shows on out / lse; backward reads a clean one
    o_b = bf(bf(p_und) @ V) if mut == "delta_undropped" else out
    delta = (dO * o_b).sum(-1, keepdim=True)
    pr = torch.exp(s * scale - lse[..., None])
    dp = dO @ V.transpose(2, 3)
    ds = bf(pr * (dp * f_bwd - delta) * scale)
    pb = bf(pr * f_bwd)
    res["dq"] = back(ds @ Kt, BF)
    if mut == "skip_last_query_block":
        last = (Nq - 1) // 64 * 64
        ds, pb = ds.clone(), pb.clone()
        ds[:, :, last:] = 0
        pb[:, :, last:] = 0
    res["dk"] = back(ds.transpose(2, 3) @ Q, BF)
    res["dv"] = back(pb.transpose(2, 3) @ dO, BF)
    return res


# ---- the fp32 kernels ---------------------------------------------------------------------------------------------------------
def fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 is exact in fp64, and one fp64 sum rounded to fp32 follows"""
    return (a.double() * b.double() + c.double()).float()


def chain(a, b, dim_a, dim_b):
    """sum_i a[i] * b[i] as the kernels' `acc += a * b` loop: one fma per term, in index order.  a and b are indexed along
    dim_a / dim_b and broadcast against each other otherwise."""
    acc = None
    for i in range(a.shape[dim_a]):
        x, y = a.select(dim_a, i), b.select(dim_b, i)
        acc = fma(x, y, torch.zeros(torch.broadcast_shapes(x.shape, y.shape)) if acc is None else acc)
    return acc


def wave_sum(x):
    """x [..., N] -> [...]: lane l sums elements l, l + 64, ... in order, then the xor butterfly of mm_common.h (32, 16, .. 1)"""
    N = x.shape[-1]
    pad = (N + 63) // 64 * 64 - N
    x = torch.nn.functional.pad(x, (0, pad)).reshape(*x.shape[:-1], -1, 64)
    lanes = torch.zeros(*x.shape[:-2], 64)
    for t in range(x.shape[-2]):
        lanes = lanes + x[..., t, :]
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[..., idx ^ o]
    return lanes[..., 0]


def emulate_f32(q, k, v, do, scale, keep, p):
    """xattn_f32_q_kernel (both modes) and xattn_f32_kv_kernel: every dot product an fp32 chain over d, over the keys or over
    the queries, in index order; the softmax sum and delta per lane and then across the wave."""
    Q, Kt, V, dO = hm(q), hm(k), hm(v), hm(do)
    f = keep.float() * XC.inv_keep(p)
    s = chain(Q[:, :, :, None, :], Kt[:, :, None, :, :], -1, -1)          # [n, H, Nq, Nkv]
    ss = s * scale
    mx = ss.amax(-1, keepdim=True)
    e = torch.exp(ss - mx)
    tot = wave_sum(e)[..., None]
    sc = e * (1.0 / tot) * f
    out = chain(sc[..., None], V[:, :, None, :, :], 3, 3)                 # over the keys -> [n, H, Nq, D]
    lse = (mx + torch.log(tot))[..., 0]
    dl = wave_sum(dO * out)[..., None]
    dpv = chain(dO[:, :, :, None, :], V[:, :, None, :, :], -1, -1)
    pr = torch.exp(s * scale - lse[..., None])
    ds = pr * (dpv * f - dl) * scale
    pd = pr * f
    dq = chain(ds[..., None], Kt[:, :, None, :, :], 3, 3)
    dk = chain(ds[..., None], Q[:, :, :, None, :], 2, 2)                  # over the queries -> [n, H, Nkv, D]
    dv = chain(pd[..., None], dO[:, :, :, None, :], 2, 2)
    return {"out": back(out, F32), "lse": lse, "dq": back(dq, F32), "dk": back(dk, F32), "dv": back(dv, F32)}


# ---- shared inputs and references ----------------------------------------------------------------------------------------------
VARIANTS = sorted({(c["shape"], c["dtype"], c["mag"]) for c in XC.CASES}, key=str)


@functools.lru_cache(maxsize=None)
def operands(shape, dtype, mag):
    return XC.make_operands(dict(shape=shape, dtype=dtype, mag=mag))


@functools.lru_cache(maxsize=None)
def problem(shape, dtype, mag, p, seed=1234, offset=7):
    """operands, the keep mask and the fp64 reference of one case: computed once, shared, never modified"""
    q, k, v, do = operands(shape, dtype, mag)
    n, Nq, Nkv, H, D = shape
    keep = XC.keep_mask(seed, offset, n, H, Nq, Nkv, p)
    return q, k, v, do, keep, XC.reference(q, k, v, do, D ** -0.5, keep, p)


CONTRACT = {(c["shape"], c["dtype"], c["mag"], c["p"]): (c["seed"], c["offset"]) for c in XC.CASES}      # what the GPU test runs


@functools.lru_cache(maxsize=None)
def emulated(shape, dtype, mag):
    """{p: {quantity: err / (u E)}} of the clean emulation at the four rates, each held to the constants; a contract case runs
    with its own (seed, offset)"""
    out = {}
    for i, p in enumerate(PS):
        seed, offset = CONTRACT.get((shape, dtype, mag, p), XC.SEEDS[i % len(XC.SEEDS)])
        q, k, v, do, keep, ref = problem(shape, dtype, mag, p, seed, offset)
        res = (emulate_bf16 if dtype == BF else emulate_f32)(q, k, v, do, shape[4] ** -0.5, keep, p)
        out[p] = XC.check_all(res, ref, dtype, None, c=XC.C[XC.path_of(dtype)])
    return out


def measured(path, nm):
    return path == "f32" or nm == "lse"          # 4x the emulation; the others (bf16 out, dq, dk, dv) are the derived 4


@pytest.mark.parametrize("variant", VARIANTS, ids=[f"{XC.path_of(d)}-" + "x".join(map(str, s)) + f"-{m}" for s, d, m in VARIANTS])
def test_emulation_passes_at_the_constants(variant):
    """at all four rates; on the (case, p) pairs the GPU test runs, with the 4x margin (bf16: within the derivation's 3 u E)"""
    path = XC.path_of(variant[1])
    for p, ratios in emulated(*variant).items():
        for nm, r in ratios.items():
            if not measured(path, nm):
                assert r <= 3.0, f"{nm} at p = {p}: {r:.3g} is past the 3 u E of the derivation"
            elif (*variant, p) in CONTRACT:
                assert 4.0 * r <= XC.C[path][nm], f"{nm} at p = {p}: the emulation's {r:.3g} leaves no 4x margin under c"


def test_constants_are_the_smallest_powers_of_two_over_the_contract_cases():
    """Every lse and fp32 constant is the smallest power of two >= 4x the emulation's worst ratio over the contract cases, no
    larger; `pytest -s` prints those ratios, the figures beside xattn_check.C.  (Runs whatever emulation is not cached yet.)"""
    worst = {}
    for variant in VARIANTS:
        for p, ratios in emulated(*variant).items():
            if (*variant, p) in CONTRACT:
                for nm, r in ratios.items():
                    key = XC.path_of(variant[1]), nm
                    worst[key] = max(worst.get(key, (0.0,)), (r, variant[0], variant[2], p))
    assert len(worst) == 10
    for (path, nm), (r, shape, mag, p) in sorted(worst.items()):
        c = XC.C[path][nm]
        print(f"\n  emulation {path}/{nm}: worst err/(u E) = {r:.3g} at {'x'.join(map(str, shape))} {mag} p={p}, c = {c}", end="")
        if measured(path, nm):
            # (1.25: room for another machine's exp / log and matmul order in the emulation, so a ratio near a power of two
            # does not flip the verdict; a constant twice too large still fails)
            assert math.log2(c) % 1 == 0 and 4.0 * r <= c < 2 * 1.25 * 4.0 * r, \
                f"{path}/{nm}: c = {c} is not the smallest power of two >= 4 x {r:.3g}"
        else:
            assert c == 4.0


# ---- the mask's geometry ------------------------------------------------------------------------------------------------------
def test_keep_mask_rounds_the_key_count_to_32():
    for Nkv, same in ((33, False), (7, False), (500, True)):               # 500 rounds to 512 either way
        a = XC.keep_mask(1234, 7, 2, 2, 5, Nkv, 0.5)
        b = XC.keep_mask(1234, 7, 2, 2, 5, Nkv, 0.5, kp_multiple=16)
        assert a.shape == (2, 2, 5, Nkv) and a.dtype == torch.bool
        assert torch.equal(a, b) == same, Nkv
        assert torch.equal(a[0, 0, 0], b[0, 0, 0])                         # row 0 starts at call 0 under either rounding
    # the flat stream is the same generator: a mask row is a slice of it
    flat = XC.dropout_keep(1234, 7, 10 * 64, 0.5).view(10, 64)
    assert torch.equal(XC.keep_mask(1234, 7, 1, 2, 5, 33, 0.5).reshape(10, 33), flat[:, :33])
    # thresholds: p = 0 keeps all; the keep rate is 1 - p within 4 sigma; 64-bit seeds and offsets select another stream
    assert bool(XC.dropout_keep(5, 5, 1000, 0.0).all())
    for p in (0.1, 0.9):
        rate = float(XC.dropout_keep(2 ** 63 - 1, 2 ** 33 + 1, 1 << 16, p).float().mean())
        assert abs(rate - (1 - p)) < 4 * math.sqrt(p * (1 - p) / (1 << 16)), (p, rate)
    assert not torch.equal(XC.dropout_keep(2 ** 63 - 1, 2 ** 33 + 1, 4096, 0.5), XC.dropout_keep(2 ** 63 - 1, 1, 4096, 0.5))
    assert XC.drop_threshold(0.5) == 2 ** 31 and XC.drop_threshold(0.0) == 0 and XC.drop_threshold(1.0) == 0xFFFFFFFF


def test_exact_zero_fixture_has_dead_rows_and_keys():
    """the fixture of the GPU test's E = 0 check: (2,5,7,1,8) at p = 0.9, seed 1234, offset 7"""
    keep = XC.keep_mask(1234, 7, 2, 1, 5, 7, 0.9)
    assert int((~keep.any(-1)).sum()) == 4 and int((~keep.any(2)).sum()) == 6
    q, k, v, do, keep, ref = problem((2, 5, 7, 1, 8), BF, "randn", 0.9)
    dead_q = (~ref["rows"]).permute(0, 2, 1)                               # [n, Nq, H]
    dead_k = (~ref["keys"]).permute(0, 2, 1)
    for nm, dead in (("out", dead_q), ("dq", dead_q), ("dv", dead_k)):
        assert bool((ref[nm][dead] == 0).all()) and bool((ref["E_" + nm][dead] == 0).all()), nm
        assert bool((ref["E_" + nm][~dead] > 0).all()), nm
    res = emulate_bf16(q, k, v, do, 8 ** -0.5, keep, 0.9)
    XC.check_all(res, ref, BF, None, c=XC.C["bf16"])
    bad = dict(res, dv=res["dv"].clone())
    b, key, h = (int(x) for x in dead_k.nonzero()[0])
    bad["dv"][b, key, h, 5] = 2.0 ** -120
    with pytest.raises(AssertionError, match=rf"dv: .* where exactly 0.0 is required .*image={b}, head={h}, key={key}, d=5"):
        XC.check_all(bad, ref, BF, None, c=XC.C["bf16"])


# ---- the mistakes -----------------------------------------------------------------------------------------------------------
# name, mutation, the smallest contract case that can show it, p, argument
MUTATIONS = [
    ("the mask row of one valid query is taken from row 0", "mask_row_from_row0", (2, 5, 7, 1, 8), 0.5, 3),
    ("the backward mask is shifted by one key", "bwd_mask_shifted", (2, 5, 7, 1, 8), 0.5, None),
    ("the backward keeps with 1 instead of 1/(1-p)", "bwd_keep_unscaled", (2, 5, 7, 1, 8), 0.1, None),
    ("delta is formed from the undropped output", "delta_undropped", (2, 5, 7, 1, 8), 0.1, None),
    ("one padding key enters the softmax", "padding_key", (2, 5, 7, 1, 8), 0.0, None),
    ("the last key's V is read as zero", "last_v_zero", (2, 5, 7, 1, 8), 0.0, None),
    ("dK/dV skip the last 64-query block", "skip_last_query_block", (1, 65, 65, 2, 72), 0.0, None),
    ("the mask is indexed with KP rounded to 16", "mask_kp16", (2, 5, 7, 1, 8), 0.5, None),
    ("one head reads its neighbour's K", "neighbour_k", (1, 64, 64, 2, 64), 0.0, 1),
    ("the last slice of D = 96 is taken from the first", "slice_from_first", (2, 40, 40, 2, 96), 0.0, None),
]
TOL, TOL_LSE = 2e-2, 5e-3            # tests/test_xattn_gpu.py


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _mutated(mut, shape, p, arg):
    """-> (worst quantity, its err / (c u E), whether the rel-L2 tolerances of tests/test_xattn_gpu.py would have passed it)"""
    q, k, v, do, keep, ref = problem(shape, BF, "randn", p)
    n, Nq, Nkv, H, D = shape
    if mut == "mask_kp16":
        arg = XC.keep_mask(1234, 7, n, H, Nq, Nkv, p, kp_multiple=16)
    res = emulate_bf16(q, k, v, do, D ** -0.5, keep, p, mut, arg)
    big = {nm: math.inf for nm in XC.QUANTITIES}
    try:
        r = XC.check_all(res, ref, BF, None, c=big)
        worst_q, ratio = max(((nm, r[nm] / XC.C["bf16"][nm]) for nm in r), key=lambda x: x[1])
    except AssertionError as e:                                           # a value where E = 0 demands exactly 0: flagged outright
        assert "exactly" in str(e), e
        worst_q, ratio = str(e).split(":")[0], math.inf
    rl2 = {nm: _rel(res[nm].float(), ref[nm]) for nm in XC.QUANTITIES}
    passed = max(rl2[nm] for nm in ("out", "dq", "dk", "dv")) < TOL and rl2["lse"] < TOL_LSE
    return worst_q, ratio, passed, " ".join(f"{nm} {rl2[nm]:.1e}" for nm in XC.QUANTITIES)


RECIPE = (2, 49, 196, 2, 96)         # the geometry tests/test_xattn_gpu.py checks with rel-L2; a contract case as well


@pytest.mark.parametrize("mutation", MUTATIONS, ids=[m[1] for m in MUTATIONS])
def test_mutation_flagged(mutation):
    name, mut, shape, p, arg = mutation
    assert any(c["shape"] == shape and c["dtype"] == BF and c["p"] == p for c in XC.CASES), "not a contract case"
    worst_q, ratio, passed, rl2 = _mutated(mut, shape, p, arg)
    assert ratio > 2.0, f"{name}: worst err/(c u E) = {ratio:.2f} ({worst_q}), needs > 2"
    verdict = lambda ok: "PASSED by rel-L2 2e-2" if ok else "seen by rel-L2"
    print(f"\n  [{name}] {'x'.join(map(str, shape))} p={p}: flagged by {ratio:.1f}x c on {worst_q}; rel-L2 {rl2} -> {verdict(passed)}")
    # the same mistake at the recipe geometry (dropout mistakes at the recipe's p = 0.1): what the rel-L2 test had in front of it
    wide = (1, 130, 500, 2, 128) if mut == "skip_last_query_block" else RECIPE
    worst_q, ratio, passed, rl2 = _mutated(mut, wide, 0.1 if p > 0 else 0.0, arg)
    print(f"      at {'x'.join(map(str, wide))}: {ratio:.1f}x c on {worst_q}; rel-L2 {rl2} -> {verdict(passed)}")
