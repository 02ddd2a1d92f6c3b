"""GEMM checker: exact and per-element fp64 references, guarded operand / output placement, and the launch path a call took.

Two families of data; for the linear paths the check can be EXACT:

Exact family (`exact_problem`).  A and B hold small integers (|a|, |b| <= 8) and every row of A / column of B (row of the
[N, K] operand) is scaled by its own power of two, so the data is asymmetric: a swapped row / column, a transposed block or a
value from a neighbouring row lands with a wrong magnitude.  Bias, residual and the accumulated C are integers in the quantum
q[m, n] = 2^(r_m + c_n) of the element they meet (bias[n] in the largest quantum of its column).  `exact_reference` asserts, per
output element and in fp64 on the device, (|A|.|B| + |bias| + |res| + |C|) / q < 2^24: every fp32 partial sum is then an
integer multiple of q below 2^24 q -- exact in fp32 whatever the summation order, the K-step split or the MFMA's internal
order.  The only rounding left is the store: the expected bf16 output is fp64_exact.float().to(bf16) (one round-to-nearest-even)
and the check is bitwise equality of every element (`check_exact`).  The fp32 GEMM must equal the fp64 value itself.

Random family (`bound_reference`).  Normal operands; the error scale E is built from absolute fp64 terms, one per rounding
point: |ref| for the final bf16 rounding and K * (u32 / u) * |A|.|B| for the fp32 accumulation (one fma per product,
cdna_hip_programming.md "FP32-input MFMA").  `check_bound` is the rule of tests/kernel_check.py with c per path (`C`).
MM_GEMM_RATIO_LOG=<file> writes the worst ratio per path at exit.

Non-linear epilogues (activation, SwiGLU, RoPE, the RMSNorm prologue of the decode fusions) are checked with `check_bound`
against an fp64 reference that takes the documented bf16 rounding points of mm_hip.h from the kernel's own bf16 outputs
where they are exactly reproducible (PRE, GU, the bf16 GEMM output before RoPE); E then carries the remaining function
error (a few fp32 ulps of each operand) and the rounding points in between.

Placement.  Outputs live in NaN-sentinel storages (`Guarded`): `out_view` places C tight (ldc = N), at a
padded ldc (the logits' layout), as a column slice of a wider buffer (the fused qkv / gate|up layout) -- always with rows past
M in the same storage.  Inputs: K-contiguous operands have zeros in [K, pad8(K)) and NaN beyond, K-strided ones NaN in the
padding columns and in rows past K, bias and residual NaN past N (`kc_storage`, `ks_storage`, ...).  A read outside the
contract that reaches a stored element then fails the exact check; a write outside the output fails Guarded.verify.

`last_kernel()` is mm_get_option("gemm_last_kernel"): every case states the kernel id it expects (see mm_hip.h)."""
import math

import torch

from tests import kernel_check as KC
from tests.kernel_check import U32, Guarded, get_option, ptr, sentinel_fill, stream

BF = torch.bfloat16
U_BF = KC.U[BF]
NT, NN, TN = 0, 1, 2
EPI_BIAS, EPI_GELU_ERF, EPI_QUICK_GELU, EPI_RESIDUAL, EPI_ACCUMULATE, EPI_GELU_TANH = 1, 2, 4, 8, 16, 32
ACTS = {EPI_GELU_ERF: "erf", EPI_QUICK_GELU: "quick", EPI_GELU_TANH: "tanh"}

# kernel ids of mm_get_option("gemm_last_kernel")
V1, DMA256x128, DMA256x256, DMA128, DMA64x128, DMA64, W4, SKINNY, GEMV, F32 = 0, 1, 2, 3, 4, 5, 10, 20, 21, 30

# c per random-family path: the smallest power of two >= 2x the worst err / (u E) measured on the MI355X over the cases of
# tests/test_gemm_contract_gpu.py and the existing GEMM tests (the PR description lists the measured ratios)
C = {
    "linear": 2.0,         # every bf16 linear path of the random family (v1, DMA tiles, 4-wave, skinny, gemv_stream): measured 0.994
    "act": 2.0,            # GELU epilogues (erf, quick, tanh), with and without the kept pre-activation: measured 0.996
    "swiglu": 2.0,         # SwiGLU forward (GEMM epilogue and decode fusion) and backward: measured 0.995
    "rope": 2.0,           # RoPE epilogue (GEMM and decode fusion): measured 0.996
    "norm": 0.5,           # decode fusions with the RMSNorm prologue: measured 0.160
}

# worst err / (u E) seen per path in this process; MM_GEMM_RATIO_LOG=<file> writes them out at exit
RATIOS = KC.RatioLog("MM_GEMM_RATIO_LOG")


def pad8(n):
    return (n + 7) // 8 * 8


def pad64(n):
    return (n + 63) // 64 * 64


# ---- exact family --------------------------------------------------------------------------------------------------------
def exact_problem(M, N, K, device, seed, span=3, amp=8, c_amp=None):
    """Logical fp64 operands of C[M, N] = A[M, K] . B[N, K]^T + bias + res + c0 (B always as [N, K]; the layout only decides
    how it is stored).  Returns a dict with A, B, bias [N], res, c0 [M, N] and q [M, N] (the quantum of every element)."""
    g = torch.Generator(device=device).manual_seed(seed)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g, device=device).double()
    re, ce = ri(-span, span, (M,)), ri(-span, span, (N,))
    a = ri(-amp, amp, (M, K)) * torch.exp2(re)[:, None]
    b = ri(-amp, amp, (N, K)) * torch.exp2(ce)[:, None]
    q = torch.exp2(re[:, None] + ce[None, :])
    ca = amp if c_amp is None else c_amp
    bias = ri(-ca, ca, (N,)) * torch.exp2(re.max() + ce)
    res = ri(-ca, ca, (M, N)) * q
    c0 = ri(-ca, ca, (M, N)) * q
    return {"A": a, "B": b, "bias": bias, "res": res, "c0": c0, "q": q}


def exact_reference(p, epi=0, a=None, b=None):
    """fp64 C of the exact family for the linear epilogue flags in `epi` (bias, residual, accumulate), after asserting that
    every fp32 partial sum of every element is exact: (|A|.|B| + |bias| + |res| + |C|) / q < 2^24."""
    a = p["A"] if a is None else a
    b = p["B"] if b is None else b
    ref = a @ b.t()
    mag = a.abs() @ b.abs().t()
    if epi & EPI_BIAS:
        ref = ref + p["bias"][None, :]
        mag = mag + p["bias"].abs()[None, :]
    if epi & EPI_RESIDUAL:
        ref = ref + p["res"]
        mag = mag + p["res"].abs()
    if epi & EPI_ACCUMULATE:
        ref = ref + p["c0"]
        mag = mag + p["c0"].abs()
    worst = float((mag / p["q"]).max()) if mag.numel() else 0.0
    assert worst < 2.0 ** 24, f"exact family out of range: (|A|.|B| + ...) / q reaches {worst:.4g} >= 2^24"
    return ref


def exact_reference_chunked(a_of, b_of, M, N, K, q, chunk=8192):
    """fp64 A.B^T for operands too large to hold in fp64 at once: a_of(k0, k1) -> [M, k1-k0], b_of(k0, k1) -> [N, k1-k0]
    (bf16 or fp64 slices of the device operands); asserts the 2^24 range per element like exact_reference."""
    ref = torch.zeros(M, N, dtype=torch.float64, device=q.device)
    mag = torch.zeros_like(ref)
    for k0 in range(0, K, chunk):
        k1 = min(K, k0 + chunk)
        a, b = a_of(k0, k1).double(), b_of(k0, k1).double()
        ref += a @ b.t()
        mag += a.abs() @ b.abs().t()
    worst = float((mag / q).max())
    assert worst < 2.0 ** 24, f"exact family out of range: |A|.|B| / q reaches {worst:.4g} >= 2^24"
    return ref


def rne_bf16(ref64):
    """The one rounding of the exact family: fp64 (exact in fp32 by construction) -> fp32 -> bf16, round to nearest even."""
    return ref64.float().to(BF)


def _where(idx, shape):
    m, n = divmod(idx, shape[1]) if len(shape) == 2 else (0, idx)
    return (f"(m={m}, n={n}) [16x16 block ({m // 16}, {n // 16}), 256x256 tile ({m // 256}, {n // 256}), "
            f"K-tail/N-tail: n % 8 = {n % 8}]")


def check_exact(name, got, want):
    """Bitwise equality of every element (got, want: the same dtype)."""
    KC.check_bits(name, got, want, where=_where)


# ---- random family -------------------------------------------------------------------------------------------------------
def bound_reference(a, b, epi=0, bias=None, res=None, c0=None):
    """fp64 reference and error scale E of the bf16 GEMM with fp32 accumulation and one bf16 rounding: a [M, K], b [N, K]
    (the values the kernel reads, any dtype).  E = |ref| + K (u32 / u) |A|.|B| (the bias / residual / C adds are fp32
    roundings of partial sums already covered by the accumulation term)."""
    a, b = a.double(), b.double()
    ref = a @ b.t()
    mag = a.abs() @ b.abs().t()
    for flag, t in ((EPI_BIAS, bias), (EPI_RESIDUAL, res), (EPI_ACCUMULATE, c0)):
        if epi & flag:
            t = t.double().to(a.device)
            ref = ref + t
            mag = mag + t.abs()
    K = a.shape[1]
    E = ref.abs() + (K + 3) * (U32 / U_BF) * mag
    return ref, E


def check_bound(name, got, ref, E, c, path=None, u=U_BF):
    """The rule; the worst err / (u E) is recorded in RATIOS[path], a failure names the element's tiles."""
    return KC.check_bound(name, got, ref, E, c, u, key=path, log=RATIOS, where=_where)


# ---- non-linear references (fp64 of the function; E: its fp32 error + the documented bf16 rounding points) ---------------
FUNC = 16 * U32 / U_BF          # the activation / SiLU / RoPE arithmetic in fp32: a few ulps of each operand, with margin


def act64(x, kind):
    if kind == "erf":
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if kind == "quick":
        return x * torch.sigmoid(1.702 * x)
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def act_reference(pre, kind, res=None, round_act=False):
    """ACT of the GELU epilogues from the pre-activation `pre` (fp64, exactly what the kernel holds before the function:
    the exact fp32 sum, or the kept bf16 PRE).  round_act: the activation is rounded to bf16 before the residual add
    (mm_gemm_act_fwd with a residual: mm_gelu_fwd + mm_add).  -> (ref, E)."""
    a = act64(pre, kind)
    ref = a if res is None else a + res
    E = ref.abs() + FUNC * (pre.abs() + a.abs())
    if round_act and res is not None:
        E = E + a.abs()
    return ref, E


def silu64(x):
    return x * torch.sigmoid(x)


def swiglu_fwd_reference(gate, up):
    """ACT = bf16(bf16(silu(gate)) * up) from the bf16 gate / up (fp64 values) -> (ref, E)."""
    s = silu64(gate)
    ref = s * up
    return ref, ref.abs() + (s * up).abs() + FUNC * (gate.abs() + s.abs()) * up.abs()


def swiglu_bwd_reference(gate, up, dact):
    """dGU = [dact * up * silu'(gate) | dact * silu(gate)] from the bf16 gate / up / dact (fp64 values) -> (dg, E_dg, du, E_du)."""
    sig = torch.sigmoid(gate)
    du = dact * gate * sig
    dg = dact * up * sig * (1.0 + gate * (1.0 - sig))
    E_du = du.abs() + FUNC * (dact * gate).abs()
    E_dg = dg.abs() + FUNC * (dact * up).abs() * (1.0 + gate.abs())
    return dg, E_dg, du, E_du


def rope_reference(x, cos, sin, cols, D=128):
    """RoPE on the first `cols` columns (heads of width D) of x [M, N] (fp64 values of the bf16 GEMM output) with per-row
    tables cos / sin [M, D/2] (fp32 values) -> (ref, E); the columns past `cols` pass unchanged (E = |x|, bitwise in practice)."""
    M, N = x.shape
    ref = x.clone()
    E = x.abs().clone()
    h = x[:, :cols].reshape(M, cols // D, D)
    lo, hi = h[..., : D // 2], h[..., D // 2:]
    c, s = cos.double()[:, None, :], sin.double()[:, None, :]
    rlo, rhi = lo * c - hi * s, hi * c + lo * s
    mag = (lo * c).abs() + (hi * s).abs() + (hi * c).abs() + (lo * s).abs()
    ref[:, :cols] = torch.cat([rlo, rhi], -1).reshape(M, cols)
    E[:, :cols] = torch.cat([rlo.abs(), rhi.abs()], -1).reshape(M, cols) + FUNC * torch.cat([mag, mag], -1).reshape(M, cols)
    return ref, E


def rmsnorm_x(x, w, eps):
    """x' = rmsnorm(x) * w in fp64 (the kernel rounds bf16(x rstd) and bf16(w .) : 2 roundings, covered in E by norm_E)."""
    x = x.double()
    rs = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    return x * rs * w.double()[None, :]


def norm_E(xn, b):
    """extra E of a product x' . B^T whose x' carries two bf16 roundings and an fp32 rstd: 3 |x'|.|B|."""
    return 3.0 * (xn.abs() @ b.double().abs().t())


# ---- placement ------------------------------------------------------------------------------------------------------------
def kc_storage(vals, dtype=BF, ld=None, extra_rows=8):
    """A K-contiguous operand [R, K] in a storage [R + extra_rows, ld]: zeros in [K, pad8(K)), NaN from pad8(K) to ld and in
    the rows past R.  -> the [R, K] view (stride ld)."""
    R, K = vals.shape
    ld = ld or pad8(K) + 16
    buf = sentinel_fill(torch.empty(R + extra_rows, ld, dtype=dtype, device=vals.device))
    buf[:R, K:pad8(K)] = 0
    buf[:R, :K] = vals.to(dtype)
    return buf[:R, :K]


def ks_storage(vals, dtype=BF, ld=None, extra_rows=72):
    """A K-strided operand [K, X] in a storage [K + extra_rows, ld]: NaN in the columns [X, ld) and in the rows past K (a
    K-step read past K meets NaN, not zeros).  -> the [K, X] view (stride ld)."""
    K, X = vals.shape
    ld = ld or pad8(X) + 8
    buf = sentinel_fill(torch.empty(K + extra_rows, ld, dtype=dtype, device=vals.device))
    buf[:K, :X] = vals.to(dtype)
    return buf[:K, :X]


def vec_storage(vals, dtype=BF, extra=64):
    """bias [N] followed by NaN."""
    buf = sentinel_fill(torch.empty(vals.numel() + extra, dtype=dtype, device=vals.device))
    buf[:vals.numel()] = vals.to(dtype)
    return buf[:vals.numel()]


def rows_storage(vals, dtype=BF, ld=None, extra_rows=8):
    """residual [M, N] in a storage [M + extra_rows, ld] with NaN past N and past M."""
    M, N = vals.shape
    ld = ld or pad8(N) + 8
    buf = sentinel_fill(torch.empty(M + extra_rows, ld, dtype=dtype, device=vals.device))
    buf[:M, :N] = vals.to(dtype)
    return buf[:M, :N]


PLACEMENTS = ("tight", "pad64", "slice")


def out_view(M, N, placement, dtype=BF, device="cuda", extra_rows=8):
    """C [M, N] inside a Guarded storage of (M + extra_rows) rows: 'tight' ldc = N; 'pad64' ldc = the next multiple of 64
    (+64 when N already is one: the logits' layout); 'slice' a column slice at a 16-byte offset of a wider buffer (fused
    qkv / gate|up).  -> (view, guarded)."""
    if placement == "tight":
        ld, off = N, 0
    elif placement == "pad64":
        ld, off = pad64(N) + (64 if N % 64 == 0 else 0), 0
    else:
        off = 16 // torch.empty((), dtype=dtype).element_size()
        ld, off = pad8(off + N + 24), off
    g = Guarded((M + extra_rows) * ld, dtype, device)
    return g.view((M, N), (ld, 1), off), g


# ---- launches -------------------------------------------------------------------------------------------------------------
def last_kernel():
    return get_option("gemm_last_kernel")


def gemm(layout, a, b, M, N, K, c, bias=None, res=None, epi=0, dtype=BF):
    """mm_gemm on storage views (a, b as laid out for `layout`, c the output view); -> the kernel id it launched."""
    from multimeditron_amd._lib import call
    call("mm_gemm", KC.dt(dtype), layout, M, N, K, ptr(a), a.stride(0), ptr(b), b.stride(0), ptr(c), c.stride(0),
         ptr(bias), ptr(res), res.stride(0) if res is not None else 0, epi, stream())
    return last_kernel()


def operands(layout, a, b, dtype=BF, lda=None, ldb=None):
    """Stored operands of `layout` from the logical a [M, K], b [N, K]: NT A kc, B kc; NN A kc, B ks [K, N]; TN A ks [K, M],
    B ks [K, N]."""
    A = ks_storage(a.t(), dtype, lda) if layout == TN else kc_storage(a, dtype, lda)
    B = kc_storage(b, dtype, ldb) if layout == NT else ks_storage(b.t(), dtype, ldb)
    return A, B


def expected_kernel(layout, M, N, K, forced=0, acts=False, w4=1, gemv=True, ncu_tiles=192):
    """The kernel id gemm_plan picks for a plain mm_gemm call (csrc/mm_gemm_plan.h, with 32-bit offsets that fit): forced =
    mm_set_option("gemm_kernel"), w4 = "gemm_w4", gemv = "gemv_stream"; every other switch at its default."""
    if forced == 0 and layout == NT and M <= 16:
        return GEMV if gemv and K % 8 == 0 and M * K * 2 <= 143 * 1024 else SKINNY
    if forced == 1:
        return V1
    if 2 <= forced <= 6:
        variant = forced - 1
    else:
        t128 = -(-M // 256) * -(-N // 128)
        if t128 >= ncu_tiles:
            variant = 2 if -(-M // 256) * -(-N // 256) >= ncu_tiles else 1
        else:
            t = -(-M // 128) * -(-N // 128)
            variant = 4 if t <= 96 else (3 if t <= 320 else 0)
    if variant == 2 and w4 and K >= 192 and not acts:
        return W4
    return variant


def check_random(name, got, a, b, epi=0, bias=None, res=None, c0=None, path="linear"):
    """Random-family check of a bf16 linear result: a [M, K], b [N, K] the logical operands (any layout they were stored in)."""
    ref, E = bound_reference(a, b, epi, bias=bias, res=res, c0=c0)
    return check_bound(name, got, ref, E, C[path], path)
