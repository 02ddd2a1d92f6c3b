"""The optimizer checker has power (no GPU).  (a) A plain torch fp32 emulation of each kernel of csrc/mm_optim.hip, summed in an
order of its own, passes tests/optim_check.py with the final c of every output at the sizes tests/test_optim_contract_gpu.py
uses.  (b) Each of the usual ways such a kernel goes wrong, applied to that emulation, is flagged at those same sizes -- by the
per-element bound, by an exact check or by the sentinel a block left behind.  (c) The size lists of the GPU file reach every loop
of sumsq_kernel."""
import contextlib

import pytest
import torch

from tests import optim_check as OC
from tests import test_optim_contract_gpu as GPU
from tests.kernel_check import SENTINEL
from tests.optim_check import BF, F32, Hyper, f32

DTYPES = [BF, F32]
ids = lambda d: OC.NAME[d] if isinstance(d, torch.dtype) else None


@pytest.fixture(autouse=True)
def _emulation_log():
    OC.PREFIX[0] = "emulation."
    yield
    OC.PREFIX[0] = ""


@contextlib.contextmanager
def as_mutant():
    """what a mutant measures goes under "mutant." in the ratio log, not among the emulation's own ratios"""
    old, OC.PREFIX[0] = OC.PREFIX[0], "mutant."
    try:
        yield
    finally:
        OC.PREFIX[0] = old


# ---- emulations (mut names a deliberate mistake) -------------------------------------------------------------------------------
def emu_partial(g, nblk, mut=None):
    n, vn = g.numel(), OC.VN[g.dtype]
    g2 = g.float() ** 2
    tail = n // vn * vn
    if mut == "tail_skipped":
        g2[tail:] = 0
    b = OC.block_of(n, nblk, g.dtype)
    order = torch.argsort(b, stable=True)
    partial = torch.stack([x.flip(0).sum() for x in torch.split(g2[order], torch.bincount(b, minlength=nblk).tolist())])
    if mut == "tail_every_block":
        partial[1:] += g2[tail:].sum()
    if mut == "vector_twice":
        j = 256 * nblk if n // vn > 4 * 256 * nblk else 0          # the second vector of thread 0's unrolled body, where there is one
        partial[b[j * vn]] += g2[j * vn:(j + 1) * vn].sum()
    if mut == "slot_unwritten":
        partial.view(torch.int32)[nblk - 1] = SENTINEL[F32]
    return partial


def emu_finish(partial, max_norm, mut=None):
    nrm = partial.flip(0).sum().sqrt()
    mx = torch.tensor(max_norm, dtype=F32)
    coef = torch.minimum(torch.ones(()), mx / (nrm + 1e-6)) if max_norm > 0 else torch.ones(())
    if mut == "no_clamp" and max_norm > 0:
        coef = mx / (nrm + 1e-6)
    if mut == "no_eps" and max_norm > 0:
        coef = torch.minimum(torch.ones(()), mx / nrm)
    return torch.stack([nrm, coef])


def emu_adamw(b, h, step, c=1.0, kind="bf16", mut=None):
    """one step in torch fp32 from the `before` dict -> the `after` dict of optim_check.check_adamw"""
    g, m, v, w = b["g"].float(), b["m"], b["v"], b["w"]
    T = lambda x: torch.tensor(x, dtype=F32)
    cc = T(1.0 if mut == "clip_ignored" else c)
    gi = g * cc
    if mut == "l2_decay":
        gi = gi + T(h.wd) * w
    o1, o2 = T(1.0) - T(h.b1), T(1.0) - T(h.b2)
    bc1 = T(f32(1.0 - f32((h.b2 if mut == "bc1_from_beta2" else h.b1) ** step)))
    bc2 = T(1.0 if mut == "no_bc2" else f32(1.0 - f32(h.b2 ** step)))
    mi = T(h.b1) * m + (gi if mut == "one_minus_b1_dropped" else o1 * gi)
    gv = g if mut == "v_unclipped" else gi
    vi = T(h.b2) * v + o2 * gv * gv
    wdec = w if mut == "l2_decay" else w * (T(1.0) - T(h.lr) * T(h.wd))
    den = torch.sqrt(vi / bc2 + T(h.eps)) if mut == "eps_inside_root" else torch.sqrt(vi / bc2) + T(h.eps)
    wo = wdec - T(h.lr) * (mi / bc1) / den
    mo = m.clone() if mut == "stale_m" else mi
    vo = vi
    if mut == "tail_untouched":
        t = w.numel() // 4 * 4
        mo, vo, wo = (torch.cat([x[:t], y[t:]]) for x, y in ((mo, m), (vo, v), (wo, w)))
    if mut == "lanes_swapped":
        for x in (mo, vo, wo):
            x[[5, 6]] = x[[6, 5]]
    after = {"m": mo, "v": vo}
    if kind == "split":
        p, lo = OC.split_reference(wo)
        if mut == "lo_wraps":
            bits = wo.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
            d = bits - ((p.view(torch.int16).to(torch.int64) & 0xFFFF) << 16)
            lo = torch.where(d > 32767, d - 65536, d).to(torch.int16)
        if mut == "p_truncated":
            bits = wo.view(torch.int32)
            p = (bits >> 16).to(torch.int16).view(BF)
            lo = torch.clamp(bits & 0xFFFF, max=32767).to(torch.int16)
        after.update(p=p, lo=lo)
    else:
        after["master"] = wo
        after["p"] = wo.to(BF) if kind == "bf16" else wo.clone()
        if mut == "p_truncated":
            after["p"] = (wo.view(torch.int32) >> 16).to(torch.int16).view(BF)
    return after


def before_of(n, kind, seed, gscale=1.0, ties=False):
    pr = OC.adamw_problem(n, F32 if kind == "f32" else BF, "cpu", seed, gscale)
    if kind == "split":
        p, lo = OC.split_reference(pr["w"])
        if ties:
            OC.plant_ties(p, lo, 2 * pr["k"], min(pr["k"], 4))
        pr["w"] = OC.join_reference(p, lo)
    return pr


KINDS = ["bf16", "f32", "split"]


# ---- (a) the emulations pass ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_adamw_emulation_passes(kind):
    for n in [1, 3, 4, 5, 1027, 10007]:
        for name, (hp, steps) in GPU.HYPER.items():
            h = Hyper(*hp)
            b = before_of(n, kind, n, gscale=1e-3 if name == "eps" else 1.0, ties=(h.wd == 0))
            for step in steps:
                for c in (1.0, f32(0.37)):
                    OC.check_adamw(f"{kind} n={n} {name} step={step} c={c}", b, emu_adamw(b, h, step, c, kind), h, step, c, kind)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sumsq_emulation_passes(dtype):
    for n in GPU.SUMSQ_N[dtype]:
        for nblk in GPU.SUMSQ_NBLK:
            for exact in (False, True):
                g, q = OC.sumsq_exact_problem(n, dtype, "cpu", n) if exact else (OC.sumsq_problem(n, dtype, "cpu", n), None)
                part = emu_partial(g, nblk)
                OC.check_partial(f"n={n} nblk={nblk}", g, nblk, part, q)
                for mx in GPU.MAX_NORMS:
                    OC.check_total(f"n={n} nblk={nblk} max_norm={mx}", part, mx, emu_finish(part, mx), g, nblk, exact)


def test_sizes_reach_every_loop():
    for dtype in DTYPES:
        seen = [OC.sumsq_bodies(n, 1, dtype) for n in GPU.SUMSQ_N[dtype]]
        for want in [set(), {"tail"}, {"single"}, {"unrolled"}, {"unrolled", "single", "tail"}]:
            assert want in seen, (OC.NAME[dtype], want, seen)
    assert -(-(10007 // 4) // (2 * 256)) == 5          # n = 10007 under adamw_blocks = 2: five grid-stride trips


# ---- (b) the mutants are flagged -------------------------------------------------------------------------------------------------
ADAMW_MUTANTS = [  # (mutant, kinds, hyper set, step, c, n)
    ("eps_inside_root", KINDS, "chained", 2, 1.0, 1027),
    ("eps_inside_root", KINDS, "eps", 2, 1.0, 1027),
    ("l2_decay", KINDS, "chained", 1, 1.0, 1027),
    ("no_bc2", KINDS, "small_lr", 3, 1.0, 1027),
    ("bc1_from_beta2", KINDS, "chained", 3, 1.0, 1027),
    ("clip_ignored", KINDS, "chained", 1, f32(0.37), 1027),
    ("v_unclipped", KINDS, "chained", 1, f32(0.37), 1027),
    ("one_minus_b1_dropped", KINDS, "chained", 1, 1.0, 1027),
    ("stale_m", KINDS, "chained", 1, 1.0, 1027),
    ("tail_untouched", KINDS, "chained", 1, 1.0, 1027),
    ("tail_untouched", KINDS, "chained", 1, 1.0, 3),
    ("lanes_swapped", KINDS, "chained", 1, 1.0, 1027),
    ("p_truncated", ["bf16", "split"], "chained", 1, 1.0, 1027),
    ("lo_wraps", ["split"], "no_decay", 1, 1.0, 1027),
]


@pytest.mark.parametrize("mut,kinds,hyper,step,c,n", ADAMW_MUTANTS, ids=[f"{m[0]}-{m[2]}-n{m[5]}" for m in ADAMW_MUTANTS])
def test_adamw_mutant_is_flagged(mut, kinds, hyper, step, c, n):
    h = Hyper(*GPU.HYPER[hyper][0])
    for kind in kinds:
        b = before_of(n, kind, n, gscale=1e-3 if hyper == "eps" else 1.0, ties=(h.wd == 0))
        OC.check_adamw("emulation", b, emu_adamw(b, h, step, c, kind), h, step, c, kind)
        with pytest.raises(AssertionError), as_mutant():
            OC.check_adamw(mut, b, emu_adamw(b, h, step, c, kind, mut), h, step, c, kind)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("mut", ["tail_skipped", "tail_every_block", "vector_twice", "slot_unwritten"])
def test_sumsq_mutant_is_flagged(dtype, mut):
    for n in [9 if dtype == BF else 5, 100003]:
        for nblk in GPU.SUMSQ_NBLK:
            if mut == "tail_every_block" and nblk == 1:
                continue                                         # one block: there is no second block to add it
            g, q = OC.sumsq_exact_problem(n, dtype, "cpu", n)
            assert bool((g[n // OC.VN[dtype] * OC.VN[dtype]:] != 0).any())
            with pytest.raises(AssertionError), as_mutant():
                OC.check_partial(mut, g, nblk, emu_partial(g, nblk, mut), q)
    g = OC.sumsq_problem(100003, dtype, "cpu", 1)                # the bound alone, on random data, where a block's sum is short
    with pytest.raises(AssertionError), as_mutant():
        OC.check_partial(mut, g, 1024, emu_partial(g, 1024, mut))


@pytest.mark.parametrize("mut", ["no_clamp", "no_eps"])
def test_finish_mutant_is_flagged(mut):
    part = emu_partial(OC.sumsq_problem(1000, F32, "cpu", 3) * (1e-4 if mut == "no_eps" else 1.0), 2)
    mx = 1e6 if mut == "no_clamp" else 1e-6
    OC.check_total("emulation", part, mx, emu_finish(part, mx))
    with pytest.raises(AssertionError), as_mutant():
        OC.check_total(mut, part, mx, emu_finish(part, mx, mut))


def test_zero_gradient():
    part = emu_partial(torch.zeros(100, dtype=BF), 2)
    total = emu_finish(part, 1.0)
    OC.check_total("zeros", part, 1.0, total)
    assert float(total[0]) == 0.0 and float(total[1]) == 1.0


# ---- the integer split ---------------------------------------------------------------------------------------------------------
def test_split_reference_on_constructed_bits():
    w, lossy = OC.constructed_bits("cpu")
    p, lo = OC.split_reference(w)
    assert bool((p.view(torch.int16) == w.to(BF).view(torch.int16)).all())       # torch's own RNE agrees with the bit arithmetic
    back = OC.join_reference(p, lo)
    same = back.view(torch.int32) == w.view(torch.int32)
    assert bool((same == ~lossy).all()) and int(lossy.sum()) == 10
    assert bool((back[lossy].view(torch.int32) == OC.ulp_below(w[lossy]).view(torch.int32)).all())
    assert bool((lo[lossy] == 0x7FFF).all())
    p2, lo2 = p.clone(), lo.clone()
    OC.plant_ties(p2, lo2, 0, p2.numel())                                         # odd p, lo = -0x8000: always the lossy case
    w2 = OC.join_reference(p2, lo2)
    finite = torch.isfinite(w2)
    assert bool((OC.split_reference(w2)[1][finite] == 0x7FFF).all())
