"""The GEMM checker has power (no GPU): a plain-torch emulation of the bf16 GEMM (fp32 accumulation in 64-wide K-steps, bias /
residual / C added in fp32, one round-to-nearest-even store) passes tests/gemm_check.py in both families, and each of the usual
ways a GEMM kernel goes wrong, applied to that emulation, is flagged: by an inequality in the exact family and -- where the
mistake moves an element by more than the rounding it is allowed -- by at least 4x the path's c in the random family.  The two
rounding-mode mistakes (truncation, rounding before the residual add) move an element by at most one bf16 ulp: no per-element
error bound can see them, which is why every linear path is held to the exact family."""
import pytest
import torch

from tests import gemm_check as GC
from tests import test_gemm_contract_gpu as GPU

BF = torch.bfloat16
M, N, K = 150, 134, 200              # two 64-row / 128-column edges, N % 8 = 6 (a ragged last column group), a ragged K-step
LDR, LDC = 144, 136


def trunc_bf16(x):
    """fp32 -> bf16 by truncation (the mistake)."""
    return (x.float().contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32).to(BF)


def emulate(a, b, bias=None, res=None, c0=None, mut=None, k_tail=None):
    """C = bf16(sum of 64-wide K-step fp32 products (+ bias) (+ residual) (+ C)) for a [M, K], b [N, K] (bf16).  res is the
    residual STORAGE [M, LDR] (its first N columns are the residual).  `mut` names a deliberate mistake; k_tail holds what the
    K-contiguous storage has in [K, pad8(K)) (zeros by contract; `garbage_k_tail` reads it)."""
    Mm, Kk = a.shape
    Nn = b.shape[0]
    af, bf = a.float(), b.float()
    if mut == "garbage_k_tail":
        af = torch.cat([af, k_tail.float()], 1)
        bf = torch.cat([bf, torch.ones(Nn, k_tail.shape[1])], 1)
        Kk = af.shape[1]
    if mut == "off_by_one_row":                   # the last row of the M edge computed from the row before it
        af = af.clone()
        af[Mm - 1] = af[Mm - 2]
    acc = torch.zeros(Mm, Nn)
    steps = list(range(0, Kk, 64))
    if mut == "drop_last_kstep":
        steps = steps[:-1]
    for k0 in steps:
        acc += af[:, k0:k0 + 64] @ bf[:, k0:k0 + 64].t()
    if mut == "transposed_block":                 # one 16x16 block of the output stored transposed
        blk = acc[32:48, 16:32].clone()
        acc[32:48, 16:32] = blk.t()
    if bias is not None:
        bv = bias.float().clone()
        if mut == "bias_wrong_group":             # the ragged-N scalar tail takes the bias of the previous 4-column group
            n0 = Nn - Nn % 4
            bv[n0:] = bias.float()[n0 - 4:Nn - 4]
        acc = acc + bv[None, :]
    if mut == "round_before_residual":
        acc = acc.to(BF).float()
    if res is not None:
        r = res.reshape(-1)[: Mm * Nn].view(Mm, Nn) if mut == "residual_stride" else res[:, :Nn]
        acc = acc + r.float()
    if c0 is not None:
        acc = acc + c0.float()
        if mut == "accumulate_twice":
            acc = acc + c0.float()
    return trunc_bf16(acc) if mut == "truncate" else acc.to(BF)


MUTATIONS = ["truncate", "round_before_residual", "drop_last_kstep", "garbage_k_tail", "transposed_block", "off_by_one_row",
             "bias_wrong_group", "residual_stride", "accumulate_twice"]
ROUNDING_ONLY = {"truncate", "round_before_residual"}
EPI = GC.EPI_BIAS | GC.EPI_RESIDUAL | GC.EPI_ACCUMULATE


def _exact_case():
    p = GC.exact_problem(M, N, K, "cpu", 11)
    a, b = p["A"].to(BF), p["B"].to(BF)
    assert torch.equal(a.double(), p["A"]) and torch.equal(b.double(), p["B"])      # bf16-exact operands
    res = torch.full((M, LDR), float("nan")).to(BF)
    res[:, :N] = p["res"].to(BF)
    res[:, N:] = (p["res"][:, : LDR - N] * 3).to(BF)       # the storage's padding columns: finite values, not the residual
    return p, a, b, p["bias"].to(BF), res, p["c0"].to(BF)


def _random_case():
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(M, K, generator=g).to(BF), torch.randn(N, K, generator=g).to(BF)
    bias, c0 = torch.randn(N, generator=g).to(BF), torch.randn(M, N, generator=g).to(BF)
    res = torch.randn(M, LDR, generator=g).to(BF)
    return a, b, bias, res, c0


def test_emulation_passes_both_families():
    p, a, b, bias, res, c0 = _exact_case()
    got = emulate(a, b, bias, res, c0)
    GC.check_exact("emulation", got, GC.rne_bf16(GC.exact_reference(p, EPI)))
    a, b, bias, res, c0 = _random_case()
    got = emulate(a, b, bias, res, c0)
    ref, E = GC.bound_reference(a, b, EPI, bias=bias, res=res[:, :N], c0=c0)
    assert GC.check_bound("emulation", got, ref, E, GC.C["linear"]) <= GC.C["linear"] / 2


@pytest.mark.parametrize("mut", MUTATIONS)
def test_exact_family_flags(mut):
    p, a, b, bias, res, c0 = _exact_case()
    tail = torch.full((M, 8 - K % 8 if K % 8 else 8), 1.0).to(BF)
    got = emulate(a, b, bias, res, c0, mut=mut, k_tail=tail)
    with pytest.raises(AssertionError, match="differ from the exact result"):
        GC.check_exact(mut, got, GC.rne_bf16(GC.exact_reference(p, EPI)))


@pytest.mark.parametrize("mut", [m for m in MUTATIONS if m not in ROUNDING_ONLY])
def test_random_family_flags_by_4c(mut):
    a, b, bias, res, c0 = _random_case()
    tail = torch.full((M, 8), 1.0).to(BF)
    got = emulate(a, b, bias, res, c0, mut=mut, k_tail=tail)
    ref, E = GC.bound_reference(a, b, EPI, bias=bias, res=res[:, :N], c0=c0)
    c = GC.C["linear"]
    with pytest.raises(AssertionError):
        GC.check_bound(mut, got, ref, E, c)
    worst = float(((got.double() - ref).abs() / (GC.U_BF * E)).max())
    assert worst >= 4 * c, f"{mut}: worst err/(u E) {worst:.3g} < 4c = {4 * c}"


def test_write_into_ldc_padding_caught():
    g = GC.Guarded(M * LDC, BF, "cpu")
    C = g.view((M, N), (LDC, 1))
    C.copy_(emulate(*_random_case()))
    g.verify("clean")
    g.buf[g.pad + 5 * LDC + N] = 0                      # one store past N in row 5
    with pytest.raises(AssertionError, match="write outside the output"):
        g.verify("C")
    g2 = GC.Guarded(M * LDC, BF, "cpu")
    C2 = g2.view((M, N), (LDC, 1))
    C2[: M - 1].copy_(emulate(*_random_case())[: M - 1])  # the last row never stored
    with pytest.raises(AssertionError, match="never written"):
        g2.verify("C")


def test_exact_generator_range_check():
    p = GC.exact_problem(64, 64, 14336, "cpu", 3)
    GC.exact_reference(p, EPI)                           # the step's largest K at the default amplitude: in range
    big = GC.exact_problem(8, 8, 4096, "cpu", 3, amp=255)
    with pytest.raises(AssertionError, match="out of range"):
        GC.exact_reference(big)


def test_placements_and_operand_storages():
    for place in GC.PLACEMENTS:
        C, g = GC.out_view(5, 12, place, device="cpu")
        assert C.stride(0) % 4 == 0 and (C.data_ptr() % 16 == 0 or place != "slice" or C.data_ptr() % 8 == 0)
        C.fill_(1.0)
        g.verify(place)
    a = torch.arange(3 * 13, dtype=torch.float32).view(3, 13)
    s = GC.kc_storage(a)
    full = s.as_strided((4, s.stride(0)), (s.stride(0), 1))
    assert torch.equal(s.float(), a) and bool((full[:3, 13:16] == 0).all()) and bool(full[:3, 16:].float().isnan().all())
    assert bool(full[3].float().isnan().all())
    t = GC.ks_storage(a.t())
    rows = t.as_strided((14, t.stride(0)), (t.stride(0), 1))
    assert bool(rows[:13, 3:].float().isnan().all()) and bool(rows[13].float().isnan().all())


# ---- the GPU module's case list covers the matrix -------------------------------------------------------------------------------
TILED = (GC.V1, GC.DMA256x128, GC.DMA256x256, GC.DMA128, GC.DMA64x128, GC.DMA64, GC.W4)
LAYOUTS = {"NT", "NN", "TN"}
LIN_EPIS = {"epi:" + e for e in GPU.BASE_EPIS}
ACT_EPIS = {"epi:" + e for e in GPU.ACT_EPIS}
NCLS = {"n8", "n4", "nodd"}
KCLS = {"k64", "kstep", "k8", "ksmall"}


def required(kid):
    if kid in TILED:
        need = LAYOUTS | LIN_EPIS | NCLS | (KCLS - {"ksmall"} if kid == GC.W4 else KCLS) | {"grid:single", "grid:multi"}
        if kid in (GC.DMA256x256, GC.W4):
            need |= {"grid:half"}
        return need if kid == GC.W4 else need | ACT_EPIS
    if kid == GC.SKINNY:
        return {"NT"} | LIN_EPIS | ACT_EPIS | NCLS | KCLS
    if kid == GC.GEMV:                                    # gemv_stream_kernel takes K % 8 == 0 only (else gemm_skinny_kernel)
        return {"NT"} | LIN_EPIS | ACT_EPIS | NCLS | (KCLS - {"k8"})
    return LAYOUTS | LIN_EPIS | NCLS | KCLS                # fp32


@pytest.mark.parametrize("kid", list(TILED) + [GC.SKINNY, GC.GEMV, GC.F32])
def test_gpu_cases_cover_the_matrix(kid):
    seen = set()
    for c in GPU.CASES:
        if c["kid"] == kid:
            seen |= GPU.edge_classes(c)
    missing = required(kid) - seen
    assert not missing, f"kernel {kid}: no case for {sorted(missing)}"


def test_gpu_module_covers_every_path():
    ids = {c["kid"] for c in GPU.CASES} | {r[-1] for r in GPU.REAL} | {t[-1] for t in GPU.THRESH}
    assert set(TILED) | {GC.SKINNY, GC.GEMV, GC.F32} <= ids
    # both sides of every 32-bit offset threshold
    assert {t[-1] for t in GPU.THRESH if "below" in t[0]} >= {GC.DMA64x128, GC.GEMV}
    assert {t[-1] for t in GPU.THRESH if "at 4 GiB" in t[0]} >= {GC.V1, GC.SKINNY}
