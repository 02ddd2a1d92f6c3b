"""The xIELU checker itself (CPU, no kernel runs): its fp64 references against torch autograd of HF's `_xielu_python` formula, the
kernel mistakes it flags, and the fp32 emulation whose ratios fixed the constants c of tests/xielu_check.py."""
import pytest
import torch

from tests import xielu_check as XC
from tests.kernel_check import U

BF, F32 = XC.BF, XC.F32


def hf64(x, ap_raw, an_raw, beta, eps):
    """HF 5.15 activations.py XIELUActivation._xielu_python, in float64"""
    alpha_p = torch.nn.functional.softplus(ap_raw)
    alpha_n = beta + torch.nn.functional.softplus(an_raw)
    return torch.where(x > 0, alpha_p * x * x + beta * x, (torch.expm1(torch.min(x, eps)) - x) * alpha_n + beta * x)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("case", list(XC.ALPHA_CASES))
def test_reference_equals_autograd_of_hf_formula(dtype, case):
    """input: x == eps, +-0, both branches, denormals, +-1e4; alpha_raw = 25 is past the softplus threshold"""
    x, dy = XC.problem(300, dtype, "cpu", 1.0, 5)
    ap, an = XC.alphas(case, dtype, "cpu")
    eps = XC.EPS[dtype]
    assert bool((x == eps).any()) and bool((x > 0).any()) and bool((x < eps).any()) and bool(((x > eps) & (x <= 0)).any())
    x64 = x.double().requires_grad_(True)
    a64, b64 = ap.double().requires_grad_(True), an.double().requires_grad_(True)
    y = hf64(x64, a64, b64, torch.tensor(XC.BETA, dtype=torch.float64), torch.tensor(eps, dtype=torch.float64))
    y.backward(dy.double())
    ref_y, _ = XC.fwd_reference(x, ap, an, XC.BETA, eps)
    ref_dx, _ = XC.bwd_reference(x, dy, ap, an, XC.BETA, eps)
    (gp, _), (gn, _) = XC.dalpha_reference(x, dy, ap, an, XC.BETA, eps)
    torch.testing.assert_close(ref_y, y.detach(), rtol=1e-13, atol=0)
    torch.testing.assert_close(ref_dx, x64.grad, rtol=1e-13, atol=0)
    tie = x == eps
    assert bool(tie.any())          # torch.min splits the tie: the gradient there carries the factor 0.5
    torch.testing.assert_close(gp, a64.grad, rtol=1e-12, atol=0)
    torch.testing.assert_close(gn, b64.grad, rtol=1e-12, atol=0)


def _setup(dtype, n=2055, scale=1.0, case="init"):
    x, dy = XC.problem(n, dtype, "cpu", scale, 11)
    ap, an = XC.alphas(case, dtype, "cpu")
    return x, dy, ap, an, XC.EPS[dtype]


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_correctly_rounded_results_pass(dtype):
    x, dy, ap, an, eps = _setup(dtype)
    y, E = XC.fwd_reference(x, ap, an, XC.BETA, eps)
    XC.bound("y", "y", dtype, y.to(dtype), y, E)
    dx, E = XC.bwd_reference(x, dy, ap, an, XC.BETA, eps)
    XC.bound("dx", "dx", dtype, dx.to(dtype), dx, E)
    for out, (g, E) in zip(("dalpha_p", "dalpha_n"), XC.dalpha_reference(x, dy, ap, an, XC.BETA, eps)):
        XC.bound(out, out, dtype, g.to(dtype), g, E)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_flags_swapped_alphas(dtype):
    x, dy, ap, an, eps = _setup(dtype)
    y, E = XC.fwd_reference(x, ap, an, XC.BETA, eps)
    wrong, _ = XC.fwd_reference(x, an, ap, XC.BETA, eps)
    with pytest.raises(AssertionError):
        XC.bound("y", "y", dtype, wrong.to(dtype), y, E)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_flags_missing_half_at_the_tie(dtype):
    x, dy, ap, an, eps = _setup(dtype)
    dx, E = XC.bwd_reference(x, dy, ap, an, XC.BETA, eps)
    a_n = XC.BETA + XC.sp64(an.double())
    wrong = torch.where(x == eps, dy.double() * (a_n * (torch.exp(x.double()) - 1.0) + XC.BETA), dx)      # m = 1 at the tie
    with pytest.raises(AssertionError):
        XC.bound("dx", "dx", dtype, wrong.to(dtype), dx, E)


def test_flags_unrounded_eps_in_a_bf16_model():
    """eps taken as -1e-6 where the model's buffer holds bf16(-1e-6): x == eps is then x > eps, the gradient loses exp(x) / 2"""
    x, dy, ap, an, eps = _setup(BF)
    dx, E = XC.bwd_reference(x, dy, ap, an, XC.BETA, eps)
    wrong, _ = XC.bwd_reference(x, dy, ap, an, XC.BETA, -1e-6)
    with pytest.raises(AssertionError):
        XC.bound("dx", "dx", BF, wrong.to(BF), dx, E)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_flags_dropped_softplus_derivative(dtype):
    x, dy, ap, an, eps = _setup(dtype)
    refs = XC.dalpha_reference(x, dy, ap, an, XC.BETA, eps)
    for out, raw, (g, E) in zip(("dalpha_p", "dalpha_n"), (ap, an), refs):
        wrong = g / XC.sp_grad64(raw.double())
        with pytest.raises(AssertionError):
            XC.bound(out, out, dtype, wrong.to(dtype), g, E)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_flags_sum_that_skips_the_tail(dtype):
    """n = 2055: the last 2055 % VN elements belong to the scalar tail; random values there (the planted edge values would make it easy)"""
    n = 2055
    g = torch.Generator().manual_seed(3)
    x, dy = torch.randn(n, generator=g).to(dtype), torch.randn(n, generator=g).to(dtype)
    ap, an = XC.alphas("init", dtype, "cpu")
    eps = XC.EPS[dtype]
    k = n - n % XC.VN[dtype]
    full = XC.dalpha_reference(x, dy, ap, an, XC.BETA, eps)
    cut = XC.dalpha_reference(x[:k], dy[:k], ap, an, XC.BETA, eps)
    flagged = 0
    for out, (gr, E), (w, _) in zip(("dalpha_p", "dalpha_n"), full, cut):
        try:
            XC.bound(out, out, dtype, w.to(dtype), gr, E)
        except AssertionError:
            flagged += 1
    assert flagged >= 1        # a tail of 7 (3) random elements holds terms of both sums with overwhelming probability; one suffices


def test_launch_geometry():
    assert [XC.blocks(n) for n in (0, 1, 2048, 2049, 300001)] == [0, 1, 1, 2, 147]
    assert XC.iters(XC.WG_ELEMS * XC.MAX_BLOCKS) == 1 and XC.iters(XC.N_ITERS2) == 2
    assert XC.blocks(XC.N_ITERS2) == 2049 and XC.blocks(XC.N_REDUCE_PASSES) == 601
    assert XC.blocks(8192 * 21504) == 4096 and XC.iters(8192 * 21504) == 21


def test_emulation_ratios_fix_the_constants():
    """The fp32 emulation of the documented operation order over the contract test's inputs: every constant admits it with the
    rule's factor of two (c >= 2x the worst ratio).  The ratios are printed (pytest -s) and stand beside the constants."""
    XC.PREFIX[0] = "xielu_emulation"
    try:
        worst = {}
        for dtype in (BF, F32):
            for n in XC.NS + (XC.N_REDUCE_PASSES,):
                for scale, case, acc in XC.contract_cases(n):
                    x, dy = XC.problem(n, dtype, "cpu", scale, n)
                    ap, an = XC.alphas(case, dtype, "cpu")
                    eps = XC.EPS[dtype]
                    op, on = XC.old_values(dtype, "cpu") if acc else (None, None)
                    y = XC.emulate_fwd(x, ap, an, XC.BETA, eps)
                    dx, gp, gn = XC.emulate_bwd(x, dy, ap, an, XC.BETA, eps, op, on)
                    ry, Ey = XC.fwd_reference(x, ap, an, XC.BETA, eps)
                    rdx, Edx = XC.bwd_reference(x, dy, ap, an, XC.BETA, eps)
                    (rp, Ep), (rn, En) = XC.dalpha_reference(x, dy, ap, an, XC.BETA, eps, op, on)
                    for out, got, ref, E in (("y", y, ry, Ey), ("dx", dx, rdx, Edx), ("dalpha_p", gp, rp, Ep), ("dalpha_n", gn, rn, En)):
                        r = XC.bound(f"{out} n={n} scale={scale} {case} acc={acc}", out, dtype, got, ref, E)
                        worst[(out, dtype)] = max(worst.get((out, dtype), 0.0), r)
        for (out, dtype), r in sorted(worst.items(), key=str):
            print(f"emulation {out} {XC.NAME[dtype]}: worst err/(u E) = {r:.3f}, c = {XC.c_of(out, dtype)}")
            assert 2.0 * r <= XC.c_of(out, dtype) or (dtype == BF and out in ("y", "dx")), (out, dtype, r)
        for out in ("y", "dx"):       # one rounding of a value whose fp32 error E already counts: at most 1 (+ nothing: E holds the rest)
            assert worst[(out, BF)] <= 1.0 and XC.c_of(out, BF) == 2.0
    finally:
        XC.PREFIX[0] = "xielu"
