"""mm_gemm_mx8 (MXFP8 x MXFP8 on the block-scaled MFMA) held to exact results and to a per-element fp64 bound.

C = bf16(A' W'^T + bias + residual) with A', W' the matrices mm_dequant_mxfp8 returns for the two packed buffers (the quantiser
itself is held bit-exact by tests/test_w8_contract_gpu.py).

Exact family (tests/gemm_check.py): integers |a|, |b| <= 8 times a power of two per row are e4m3 numbers under MX scales --
dequant(quant(.)) must return them unchanged, asserted first -- and every fp32 partial sum is exact, so C must equal
fp64.float().to(bf16) bit for bit.  The first case, M = N = 16, K = 128, is ONE MFMA per output tile: the check of the operand
and scale lane maps.  `_varying_problem` gives every 32-block of a row its own exponent inside [-6, 6]: row exponent + a per-block
exponent s (+s in A, -s in W, so the product's quantum stays 2^(r_m + c_n)) + an independent 0 / 1 per (row, block), which keeps a
scale byte taken from another block visible even when both operands make the same mistake; (|A|.|B| + ...) / q < 2^24 holds
with q = 2^(r_m + c_n), the smallest quantum.  MEASURED on the MI355X: these cases pass bitwise -- the scaled MFMA sums blocks of
different scale exactly when the sum is representable.

Random family: normal operands and W8.sample_matrix (zero blocks, negative zeros, e4m3 subnormals, magnitudes over 2^+-20)
quantised by the library; reference fp64 A'.W'^T, E = |ref| + (K + 3) (u32 / u) |A'|.|W'| (gemm_check.bound_reference).
C_MX8: the smallest power of two >= 2x the worst err / (u E) measured on the MI355X over these cases (MM_GEMM_RATIO_LOG, path
"mx8"): measured 1.149 (M = 255, N = 1000, K = 384 on W8.sample_matrix operands; 0.93 on normal ones), so c = 4 -- above the
bf16 GEMM's 0.994: on blocks whose magnitudes spread over 2^+-20 the instruction's sum over its 128 k is not the chain of fp32
fmas the E term counts, but it stays inside twice that.

Placement: C tight / padded ldc / column slice in NaN-sentinel storages, the packed buffers in storages of exactly
mm_mxfp8_bytes between bands of 0xFF bytes (an e4m3 NaN, an E8M0 NaN), residual aliasing C.  The grid is one workgroup per tile
(not persistent), so there is no tiles-over-workgroups case."""
import pytest
import torch

from multimeditron_amd import kernels as K
from multimeditron_amd._lib import call
from tests import gemm_check as GC
from tests import kernel_check as KC
from tests import w8_check as W8
from tests.kernel_check import ptr, stream

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
MX8 = 23                      # "gemm_last_kernel" of mm_gemm_mx8
C_MX8 = 4.0
BIAS, RES = GC.EPI_BIAS, GC.EPI_RESIDUAL
PAD = 4096                    # bytes of 0xFF on either side of a packed buffer


class Packed:
    """mm_quant_mxfp8(x) in a storage of exactly mm_mxfp8_bytes between two bands of 0xFF bytes."""

    def __init__(self, x):
        R, Kd = x.shape
        self.n = K.mxfp8_bytes(R, Kd)
        self.buf = torch.full((PAD + self.n + PAD,), 0xFF, dtype=torch.uint8, device="cuda")
        self.view = self.buf[PAD:PAD + self.n]
        assert self.view.data_ptr() % 16 == 0
        call("mm_quant_mxfp8", x.data_ptr(), x.stride(0), R, Kd, self.view.data_ptr(), stream())
        torch.cuda.synchronize()
        self.keep = self.view.clone()
        self.dq = K.dequant_mxfp8(self.view, R, Kd)

    def verify(self, name):
        assert bool((self.buf[:PAD] == 0xFF).all()) and bool((self.buf[PAD + self.n:] == 0xFF).all()), f"{name}: write outside the packed buffer"
        assert torch.equal(self.view, self.keep), f"{name}: the packed buffer changed"


def _launch(M, N, Kd, pa, pw, c, bias=None, res=None, epi=0):
    rc = KC.rc("mm_gemm_mx8", M, N, Kd, ptr(pa), ptr(pw), ptr(bias), ptr(res), res.stride(0) if res is not None else 0, ptr(c), c.stride(0), epi)
    torch.cuda.synchronize()
    return rc


def _varying_problem(M, N, Kd, seed):
    """exact_problem with per-block exponents (module docstring); q = 2^(re + ce) is the smallest quantum of every element."""
    p = GC.exact_problem(M, N, Kd, "cuda", seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    nb = Kd // 32
    s = torch.randint(-2, 3, (nb,), generator=g, device="cuda").double()
    ja = torch.randint(0, 2, (M, nb), generator=g, device="cuda").double()
    jb = torch.randint(0, 2, (N, nb), generator=g, device="cuda").double()
    p["A"] = (p["A"].view(M, nb, 32) * torch.exp2(s[None, :] + ja)[:, :, None]).view(M, Kd)
    p["B"] = (p["B"].view(N, nb, 32) * torch.exp2(-s[None, :] + jb)[:, :, None]).view(N, Kd)
    return p


def _run_exact(p, M, N, Kd, epi, placement, alias=False):
    a, b = GC.kc_storage(p["A"]), GC.kc_storage(p["B"])
    pa, pw = Packed(a), Packed(b)
    # the operands are e4m3 numbers under their MX scales: the quantiser changes nothing
    KC.check_bits("dequant(quant(A))", pa.dq, p["A"].to(BF))
    KC.check_bits("dequant(quant(B))", pw.dq, p["B"].to(BF))
    want = GC.rne_bf16(GC.exact_reference(p, epi))
    c, g = GC.out_view(M, N, placement)
    bias = GC.vec_storage(p["bias"]) if epi & BIAS else None
    res = None
    if epi & RES:
        if alias:
            c.copy_(p["res"].to(BF))
            res = c
        else:
            res = GC.rows_storage(p["res"])
    assert _launch(M, N, Kd, pa.view, pw.view, c, bias, res, epi) == 0
    assert GC.last_kernel() == MX8
    g.verify("C")
    pa.verify("packedA")
    pw.verify("packedW")
    GC.check_exact(f"mx8 exact M={M} N={N} K={Kd} epi={epi} {placement}", c, want)


# ---- exact family ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", [0, BIAS | RES])
def test_one_mfma_per_tile_is_the_lane_map(epi):
    _run_exact(GC.exact_problem(16, 16, 128, "cuda", 11), 16, 16, 128, epi, "tight")


EXACT = [  # M, N, K, epi, placement, residual aliases C
    (1, 8, 128, BIAS, "tight", False),
    (17, 136, 384, RES, "pad64", False),
    (255, 264, 128, 0, "slice", False),
    (257, 1000, 384, BIAS | RES, "tight", True),
    (257, 264, 4096, 0, "pad64", False),
    (17, 1000, 4096, BIAS, "slice", False),
    (1, 136, 4096, RES, "tight", True),
    (255, 8, 384, 0, "pad64", False),
    (257, 136, 128, BIAS | RES, "slice", True),
    (17, 264, 384, BIAS, "tight", False),
    (255, 1000, 128, RES, "slice", False),
    (17, 136, 3584, BIAS | RES, "pad64", False),      # a width whose layout has padding slots (per = 14, sper = 16)
]


@pytest.mark.parametrize("M,N,K_,epi,placement,alias", EXACT)
def test_exact_family(M, N, K_, epi, placement, alias):
    _run_exact(GC.exact_problem(M, N, K_, "cuda", M * 31 + N * 7 + K_), M, N, K_, epi, placement, alias)


@pytest.mark.parametrize("M,N,K_,epi", [(16, 16, 128, 0), (17, 136, 384, BIAS | RES), (257, 264, 4096, 0), (255, 1000, 384, RES),
                                         (17, 8, 3584, BIAS)])
def test_scales_that_vary_along_k(M, N, K_, epi):
    _run_exact(_varying_problem(M, N, K_, M + N + K_), M, N, K_, epi, "slice")


# ---- random family -----------------------------------------------------------------------------------------------------------------
def _random_operand(R, Kd, seed, kind):
    if kind == "sample":
        return W8.sample_matrix(R, Kd, seed, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(R, Kd, generator=g, device="cuda") * 0.5).to(BF)


@pytest.mark.parametrize("M,N,K_,epi,kind,placement", [
    (17, 136, 384, 0, "normal", "tight"),
    (257, 264, 4096, BIAS | RES, "normal", "pad64"),
    (255, 1000, 384, BIAS, "sample", "slice"),
    (257, 136, 4096, RES, "sample", "tight"),
    (17, 264, 3584, 0, "normal", "slice"),
    (1, 8, 128, BIAS | RES, "sample", "pad64"),
])
def test_random_family(M, N, K_, epi, kind, placement):
    a, w = _random_operand(M, K_, 3 * M + K_, kind), _random_operand(N, K_, 5 * N + K_ + 1, kind)
    pa, pw = Packed(GC.kc_storage(a)), Packed(GC.kc_storage(w))
    KC.check_bits("A' vs the format's reference", pa.dq, W8.roundtrip_ref(a.cpu()))
    g0 = torch.Generator(device="cuda").manual_seed(M + N)
    amp = float((pa.dq.double().abs() @ pw.dq.double().abs().t()).mean())
    bias = (torch.randn(N, generator=g0, device="cuda") * amp).to(BF) if epi & BIAS else None
    res = (torch.randn(M, N, generator=g0, device="cuda") * amp).to(BF) if epi & RES else None
    c, g = GC.out_view(M, N, placement)
    bs = GC.vec_storage(bias) if bias is not None else None
    rs = GC.rows_storage(res) if res is not None else None
    assert _launch(M, N, K_, pa.view, pw.view, c, bs, rs, epi) == 0
    g.verify("C")
    pa.verify("packedA")
    pw.verify("packedW")
    ref, E = GC.bound_reference(pa.dq, pw.dq, epi, bias=bias, res=res)
    worst = GC.check_bound(f"mx8 random M={M} N={N} K={K_} {kind}", c, ref, E, C_MX8, path="mx8")
    print(f"mx8 random M={M} N={N} K={K_} {kind}: err/(u E) = {worst:.4g}")
    # determinism: a second call returns the same bits
    c2, g2 = GC.out_view(M, N, placement)
    assert _launch(M, N, K_, pa.view, pw.view, c2, bs, rs, epi) == 0
    g2.verify("C, second call")
    KC.check_bits("two calls", c2, c.clone())


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_c_untouched():
    pk = torch.zeros(K.mxfp8_bytes(32, 4096), dtype=torch.uint8, device="cuda")
    c, g = GC.out_view(16, 16, "tight")
    assert _launch(16, 16, 96, pk, pk, c) == GC.ERR_UNSUPPORTED                                  # K % 128
    assert _launch(16, 16, 128, pk, pk, c, epi=GC.EPI_GELU_ERF) == GC.ERR_UNSUPPORTED
    assert _launch(16, 16, 128, pk, pk, c, epi=GC.EPI_ACCUMULATE) == GC.ERR_UNSUPPORTED
    assert _launch(16, 16, 128, pk, pk, c, epi=BIAS) == GC.ERR_ARG                               # no bias given
    assert _launch(0, 16, 128, pk, pk, c) == GC.ERR_ARG
    assert _launch(16, 16, 128, pk[8:], pk, c) == GC.ERR_ALIGN
    GC.untouched([g])
    assert K.gemm_mx8_supported(16, 16, 96) is not None and "96" in K.gemm_mx8_supported(16, 16, 96)
    assert K.gemm_mx8_supported(16, 16, 3584) is None and K.gemm_mx8_supported(8192, 28672, 4096) is None
