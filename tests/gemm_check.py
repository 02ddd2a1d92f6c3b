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
import ctypes
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
    "linear": 2.0,         # every bf16 linear path of the random family (v1, DMA tiles, 4-wave, skinny, gemv_stream): measured 0.994;
                           # the grouped launches (paths grouped-linear, grouped-linear-f32): 0.993, 0.075
    "act": 2.0,            # GELU epilogues (erf, quick, tanh), with and without the kept pre-activation: measured 0.996;
                           # mm_gemm_act_fwd_batched (path grouped-act): 0.995
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
    how it is stored).  Returns a dict with A, B, bias [N], res, c0 [M, N], q [M, N] (the quantum of every element) and the
    row / column exponents re [M], ce [N] behind it (q = 2^(re + ce))."""
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
    return {"A": a, "B": b, "bias": bias, "res": res, "c0": c0, "q": q, "re": re, "ce": ce}


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


# ---- grouped launches (mm_gemm_batched, mm_gemm_act_fwd_batched, mm_colsum_batched) ------------------------------------------------
# A grouped launch is held to the SAME references as the stand-alone call, problem by problem: every problem of a launch has
# its own seed (operands, bias, residual and accumulated C differ from problem to problem, so a pointer-table entry taken from
# another problem lands on foreign data), the exact family is compared bitwise and the random family under C["linear"] /
# C["act"] -- the arithmetic is mm_gemm's, so there is no constant of its own; the worst ratios are recorded under the path
# keys grouped-linear (measured 0.993 against c = 2), grouped-linear-f32 (0.075; the fp32 E counts one rounding per fma) and
# grouped-act (0.995 against c = 2) over tests/test_grouped_contract_gpu.py.  Outputs sit expert-major in ONE Guarded storage (problem p + 1's
# rows follow problem p's at a padded ld, as kernels._rows hands them over: a tile that overhangs M lands in the next problem)
# or in one Guarded storage per problem between sentinel rows.  `plan` is mm_gemm_plan: every case asserts the path it claims.
FP32 = torch.float32                             # the dtype; F32 above is the fp32 kernel's id
GROUP_MAX = 16                                   # MM_GROUP_MAX
KIND_PLAIN, KIND_ACT_FWD = 0, 1                  # mm_gemm_plan's `kind`
FAM_NONE, FAM_V1, FAM_DMA, FAM_F32 = -1, 0, 1, 5   # ... and the kernel families it reports
OK, ERR_ARG, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -3
PLAN_INTS = 26
GROUPED_PLACEMENTS = ("expert_major", "separate")


def pa(ts):
    """host array of device pointers for a grouped entry point: tensors, raw addresses or None (a NULL entry); None -> a NULL table"""
    if ts is None:
        return None
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() if isinstance(t, torch.Tensor) else t for t in ts])


def out_ld(N):
    """the padded leading dimension of a grouped output"""
    return pad8(N) + 8


def grouped_lds(layout, M, N, K):
    """(lda, ldb, ldc, ldr) of `operands`, `grouped_out` and `rows_storage` at their defaults"""
    return (pad8(M) + 8 if layout == TN else pad8(K) + 16, pad8(K) + 16 if layout == NT else pad8(N) + 8, out_ld(N), pad8(N) + 8)


def plan(dtype, layout, kind, groups, M, N, K, epi=0, ncu=0, lds=None, ptr_bits=0):
    """mm_gemm_plan under the current switches (groups = 0: the stand-alone call; ncu = 0: the current device's CUs) -> dict with
    rc, last (the kernel id, -2 = unchanged), family, tile (BM, BN of an LDS-DMA plan), grid_x, grid_y, tiles (per problem)."""
    lda, ldb, ldc, ldr = lds or grouped_lds(layout, M, N, K)
    out = (ctypes.c_int * PLAN_INTS)()
    rc = KC.lib().mm_gemm_plan(KC.dt(dtype), layout, kind, groups, M, N, K, lda, ldb, ldc, ldr if epi & EPI_RESIDUAL else 0, 0, epi, 0,
                               ptr_bits, ncu, out)
    assert rc == 0, (rc, dtype, layout, kind, groups, M, N, K)
    v = list(out)
    return dict(rc=v[0], last=v[1], family=v[2], tile=(v[5], v[6]), grid_x=v[11], grid_y=v[12], tiles=v[15] * v[16])


def grouped_problems(family, groups, M, N, K, device, seed, dtype=BF, same_a=False):
    """`groups` problems of one shape, each under its own seed -> a list of exact_problem-style dicts (fp64 values that the
    storage dtype holds exactly).  family "random": normal operands (sigma 0.5), bias / residual / C of sigma 1.  same_a: every
    problem reads problem 0's A (the patch embedding's form); an exact problem then keeps only what a plain epilogue needs."""
    out = []
    for p in range(groups):
        s = seed + 7919 * p
        if family == "exact":
            d = exact_problem(M, N, K, device, s)
            if same_a and p:
                d = {"A": out[0]["A"], "B": d["B"], "re": out[0]["re"], "ce": d["ce"], "q": torch.exp2(out[0]["re"][:, None] + d["ce"][None, :])}
        else:
            g = torch.Generator(device=device).manual_seed(s)
            r = lambda *sh: (torch.randn(*sh, generator=g, device=device) * 0.5).to(dtype).double()
            d = {"A": r(M, K), "B": r(N, K), "bias": r(N) * 2.0, "res": r(M, N) * 2.0, "c0": r(M, N) * 2.0}
            if same_a and p:
                d["A"] = out[0]["A"]
        out.append(d)
    return out


def grouped_operands(layout, probs, epi, dtype=BF, same_a=False):
    """stored operands of every problem (NaN beyond the contract: `operands`, `vec_storage`, `rows_storage`) ->
    (As, Bs, biases or None, residuals or None)"""
    As, Bs = [], []
    for p, d in enumerate(probs):
        A, B = operands(layout, d["A"], d["B"], dtype)
        As.append(As[0] if same_a and p else A)
        Bs.append(B)
    biases = [vec_storage(d["bias"], dtype) for d in probs] if epi & EPI_BIAS else None
    res = [rows_storage(d["res"], dtype) for d in probs] if epi & EPI_RESIDUAL else None
    return As, Bs, biases, res


def grouped_out(groups, M, N, place, dtype=BF, device="cuda", extra_rows=8, gap_rows=3):
    """`groups` outputs [M, N] at ld = out_ld(N).  'expert_major': ONE Guarded storage [groups * M + extra_rows, ld], problem p at
    row p * M;  'separate': one Guarded storage per problem with gap_rows sentinel rows above and below.  -> (views, guards)"""
    ld = out_ld(N)
    if place == "expert_major":
        g = Guarded((groups * M + extra_rows) * ld, dtype, device)
        return [g.view((M, N), (ld, 1), p * M * ld) for p in range(groups)], [g]
    guards = [Guarded((M + 2 * gap_rows) * ld, dtype, device) for _ in range(groups)]
    return [g.view((M, N), (ld, 1), gap_rows * ld) for g in guards], guards


def fill_c0(outs, probs, dtype=BF):
    """what C holds before an accumulating launch"""
    for c, d in zip(outs, probs):
        c.copy_(d["c0"].to(dtype))


def verify_all(name, guards, require_written=True):
    for i, g in enumerate(guards):
        g.verify(f"{name} [{i}]", require_written)


def untouched(guards):
    """a refused or empty call wrote nothing: every element of every storage is still the sentinel"""
    for g in guards:
        assert bool((KC._ints(g.buf) == KC.SENTINEL[g.dtype]).all()), "a refused or empty call wrote to its output"


def batched_args(layout, M, N, K, As, Bs, Cs, biases=None, res=None, epi=0, dtype=BF, pres=None):
    """the arguments of one mm_gemm_batched call (pres given: mm_gemm_act_fwd_batched, Cs = ACT) by name, so that a refusal
    test can replace one of them; the pointer lists take tensors, raw addresses or None."""
    return dict(dtype=KC.dt(dtype), layout=layout, groups=len(Cs), M=M, N=N, K=K, A=list(As), lda=As[0].stride(0), B=list(Bs),
                ldb=Bs[0].stride(0), C=list(Cs), ldc=Cs[0].stride(0), bias=list(biases) if biases is not None else None,
                res=list(res) if res is not None else None, ldr=res[0].stride(0) if res is not None else 0, epi=epi,
                PRE=list(pres) if pres is not None else None, ldpre=pres[0].stride(0) if pres is not None else 0, act_fwd=pres is not None)


def launch_batched(a):
    """-> the raw return code of the grouped entry point `a` (batched_args) describes"""
    if a["act_fwd"]:
        return KC.rc("mm_gemm_act_fwd_batched", a["dtype"], a["groups"], a["M"], a["N"], a["K"], pa(a["A"]), a["lda"], pa(a["B"]), a["ldb"],
                     pa(a["bias"]), pa(a["PRE"]), a["ldpre"], pa(a["C"]), a["ldc"], pa(a["res"]), a["ldr"], a["epi"])
    return KC.rc("mm_gemm_batched", a["dtype"], a["layout"], a["groups"], a["M"], a["N"], a["K"], pa(a["A"]), a["lda"], pa(a["B"]), a["ldb"],
                 pa(a["C"]), a["ldc"], pa(a["bias"]), pa(a["res"]), a["ldr"], a["epi"])


def grouped_want(family, d, epi, dtype=BF):
    """what problem `d` must give under the linear epilogue flags `epi`: ('exact', tensor of the output dtype) or
    ('bound', (ref, E)) with E in units of the output dtype's u (fp32: |ref| + (K + 3) |A|.|B| + ..., one rounding per fma)."""
    if family == "exact":
        ref = exact_reference(d, epi)
        return "exact", (ref.float() if dtype == FP32 else rne_bf16(ref))
    ref, E = bound_reference(d["A"], d["B"], epi, bias=d.get("bias"), res=d.get("res"), c0=d.get("c0"))
    if dtype == FP32:
        E = ref.abs() + (E - ref.abs()) * (U_BF / U32)
    return "bound", (ref, E)


def check_grouped(tag, family, probs, epi, outs, dtype=BF, path="grouped-linear"):
    """every problem's output against ITS reference: bitwise in the exact family, C["linear"] in the random one (recorded under
    `path`, `path`-f32 for fp32).  -> the worst ratio (0 in the exact family)."""
    worst = 0.0
    for p, (d, c) in enumerate(zip(probs, outs)):
        kind, want = grouped_want(family, d, epi, dtype)
        if kind == "exact":
            check_exact(f"{tag} problem {p}", c, want.to(c.device))
        else:
            ref, E = want
            key = path if dtype == BF else path + "-f32"
            worst = max(worst, check_bound(f"{tag} problem {p}", c, ref.to(c.device), E.to(c.device), C["linear"], key, u=KC.U[dtype]))
    return worst


def check_grouped_act(tag, family, probs, flags, kind, pres, acts, path="grouped"):
    """mm_gemm_act_fwd(_batched) per problem: PRE = bf16(X.W^T + bias) (exact family: bitwise; random: C["linear"]), ACT = act(PRE)
    (rounded to bf16 before a residual add) from the kernel's own PRE under C["act"], recorded under `path`-linear / `path`-act."""
    worst = 0.0
    for p, d in enumerate(probs):
        check_grouped(f"{tag} PRE", family, [d], flags & EPI_BIAS, [pres[p]], path=path + "-linear")
        res = d["res"].to(pres[p].device) if flags & EPI_RESIDUAL else None
        ref, E = act_reference(pres[p].double(), kind, res, round_act=True)
        worst = max(worst, check_bound(f"{tag} ACT problem {p}", acts[p], ref, E, C["act"], path + "-act"))
    return worst


def colsum_problems(groups, R, N, device, seed):
    """exact-family rows per expert, as test_colsum_exact builds them: d["res"] [R, N] are the rows, d["c0"][0] * 2^6 what `out`
    holds before an accumulating call."""
    return [exact_problem(R, N, 8, device, seed + 7919 * p, span=2) for p in range(groups)]


def colsum_storage(probs, dtype, extra_rows=4):
    """the experts' rows expert-major in ONE storage [groups * R + extra_rows, ldx] with a padded ldx: NaN in the padding columns
    and in the rows past the last expert; expert p + 1's rows follow expert p's.  -> the per-expert [R, N] views"""
    R, N = probs[0]["res"].shape
    ldx = pad8(N) + 8
    buf = sentinel_fill(torch.empty(len(probs) * R + extra_rows, ldx, dtype=dtype, device=probs[0]["res"].device))
    for p, d in enumerate(probs):
        buf[p * R:(p + 1) * R, :N] = d["res"].to(dtype)
    return [buf[p * R:(p + 1) * R, :N] for p in range(len(probs))]


def colsum_want(d, accumulate, dtype):
    """-> (what out holds before, the exact result in the output dtype) after the range assertion of the exact family"""
    base = d["c0"][0] * 2.0 ** 6 if accumulate else torch.zeros_like(d["c0"][0])
    ref = d["res"].sum(0) + base
    assert float(((d["res"].abs().sum(0) + base.abs()) / d["q"].min(0).values).max()) < 2.0 ** 24
    return base.to(dtype), (ref.float() if dtype == FP32 else rne_bf16(ref))
