"""xIELU kernel checker (csrc/mm_xielu.hip): fp64 references with per-element error scales, problems with planted edge values, guarded
launches, and a CPU fp32 emulation of the kernels' documented operation order.

Every reference takes the STORED operands (x, dy, the raw scalars in T; beta / eps as the floats the kernel receives) and returns
(ref, E) in fp64 for the rule of tests/kernel_check.py.  The rounding points, read off mm_xielu.hip (T = storage type, the rest fp32):

  scalars   ap = sp(alpha_p_raw), an = beta + sp(alpha_n_raw), sp(a) = a > 20 ? a : log1pf(expf(a))        SP ulps of sp, + 1 for the add
  em        expm1 of xm = min(x, eps) <= 0: xm > -0.35: fma(xm*xm, q(xm), xm), q a degree-5 Horner chain of fmas (truncation 1.6e-8);
            otherwise exp2(xm * log2 e) - 1.  E_em = EM |em| + 2 |xm| exp(xm): a few ulps of the result and, on the exp branch, the
            rounding of the exponent's argument (relative |xm| u32 on exp)
  y         x > 0: fma(ap, x, beta) * x;  else fma(an, em - x, beta * x);  T(.)                             one rounding to T
  dx        x > 0: dy * fma(ap + ap, x, beta);  else dy * fma(an, ge, beta), ge = em | fma(0.5, em, -0.5) | -1 for x < | == | > eps
  sums      tp = (dy * x) * x (x > 0), tn = dy * (em - x) (x <= 0), 0 otherwise; a lane adds its 8 * iters terms in element order,
            block_sum_256 (6 shuffle levels + 3 adds), the finishing launch adds ceil(nblk / 256) workgroups per lane in order and
            block_sum_256 again: depth(n) = 8 iters + 9 + ceil(nblk / 256) + 9.  Then * sp'(alpha_raw) (SP ulps), + the old value in
            fp32 when accumulating, one rounding to T.

Constants c (`C`).  y and dx in bf16 are ONE rounding of a value whose fp32 error E already counts: c = 2, the rule's factor of two over
a ratio that cannot exceed 1 by more than the fp32 terms.  For the fp32 outputs and the two scalar gradients c was fixed BEFORE any GPU
run: the smallest power of two >= 2x the worst ratio of `emulate_*` (fp32 on the CPU, the operation order above) over the inputs of
tests/test_xielu_contract_gpu.py (tests/test_xielu_check_cpu.py::test_emulation_ratios_fix_the_constants recomputes them).  The
ratios are recorded under xielu.<output>.<dtype> in the ratio log (MM_GEMM_RATIO_LOG)."""
import math

import torch

from tests.gemm_check import RATIOS
from tests.kernel_check import U, U32, check_bound

BF, F32 = torch.bfloat16, torch.float32
NAME = {BF: "bf16", F32: "f32"}
VN = {BF: 8, F32: 4}
OK, ERR_ARG, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -3
WG_ELEMS, MAX_BLOCKS = 2048, 4096        # XIELU_WG_ELEMS, XIELU_MAX_BLOCKS
SP = 8.0                                  # ulps of softplus / its derivative (expf, log1pf, a division)
EM = 4.0                                  # ulps of expm1_neg's result
FLOOR = 2.0 ** -125                       # underflow: every fp32 operation is also good to 2^-149 only (FLOOR u32), a bf16 store to
                                          # 2^-133 (FLOOR u_bf16); 4 operations per element are counted
BETA = 0.5
EPS = {F32: float(torch.tensor(-1e-6, dtype=F32)), BF: float(torch.tensor(-1e-6, dtype=BF))}      # bf16: -9.98377799987793e-07
ALPHA_INIT = (math.log(math.expm1(0.8)), math.log(math.expm1(0.8 - 0.5)))                          # HF XIELUActivation's constructor
ALPHA_CASES = {"init": ALPHA_INIT, "neg3_25": (-3.0, 25.0), "25_neg3": (25.0, -3.0)}               # 25: past the softplus threshold

# c per output (bf16, f32).  In the comments: the CPU emulation's worst ratios (bf16, f32) over the contract test's inputs, which
# fixed the constants, then the MI355X's from the ratio log of tests/test_xielu_contract_gpu.py (the worst elements come out with
# the emulation's bits).  A ratio above c is a finding to explain in E (the device's exp / log1p), not a constant to raise.
C = {
    "y": (2.0, 2.0),            # emulation 0.988, 0.991;  MI355X 0.988, 0.991
    "dx": (2.0, 2.0),           # emulation 0.996, 0.982;  MI355X 0.996, 0.982
    "dalpha_p": (2.0, 0.125),   # emulation 0.852, 0.059;  MI355X 0.852, 0.059
    "dalpha_n": (2.0, 2.0),     # emulation 0.974, 0.663 (an accumulating launch at n = 7: the one rounding of old + new);  MI355X 0.974, 0.663
}


def c_of(out, dtype):
    return C[out][0 if dtype == BF else 1]


PREFIX = ["xielu"]              # the CPU test records its emulation under "xielu_emulation" instead


def bound(name, out, dtype, got, ref, E):
    return check_bound(name, got, ref.to(got.device), E.to(got.device), c_of(out, dtype), U[dtype], key=f"{PREFIX[0]}.{out}.{NAME[dtype]}",
                       log=RATIOS)


# ---- launch geometry mirrored from mm_xielu.hip ----------------------------------------------------------------------------------
def iters(n):
    return max(1, -(-(-(-n // WG_ELEMS)) // MAX_BLOCKS))


def blocks(n):
    return 0 if n <= 0 else -(-n // (iters(n) * WG_ELEMS))


def depth(n):
    return 8 * iters(n) + 9 + -(-blocks(n) // 256) + 9


def _uscale(dtype):
    return U32 / U[dtype]


# ---- problems ----------------------------------------------------------------------------------------------------------------------
def neighbours(v, dtype):
    """the two values of `dtype` next to v (v representable)"""
    t = torch.tensor([v], dtype=dtype)
    i = t.view(torch.int16 if dtype == BF else torch.int32)
    return float((i + 1).view(dtype)), float((i - 1).view(dtype))


def edge_values(dtype):
    """+-0, eps, its two neighbours in T, denormals of both signs, +-1e4, and -100 where expm1 is exactly -1 in fp32"""
    eps = EPS[dtype]
    lo, hi = neighbours(eps, dtype)
    tiny = 2.0 ** -130 if dtype == BF else 2.0 ** -140
    return torch.tensor([0.0, -0.0, eps, lo, hi, tiny, -tiny, 1e4, -1e4, -100.0], dtype=torch.float64).to(dtype)


def problem(n, dtype, device, scale, seed):
    """x ~ N(0, 1) * scale with the edge values planted at the front and again at the very end (the scalar tail's elements when n is no
    multiple of the vector), dy ~ N(0, 1): both signs.  Stored in T."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.randn(n, generator=g) * scale).to(dtype)
    dy = torch.randn(n, generator=g).to(dtype)
    e = edge_values(dtype)
    k = min(n, e.numel())
    x[:k] = e[:k]
    if n >= 2 * e.numel():
        x[n - e.numel():] = e
    return x.to(device), dy.to(device)


def alphas(case, dtype, device):
    """the raw scalars of a case in T; "init" as HF's constructor computes them, in T's arithmetic"""
    ap, an = ALPHA_CASES[case]
    if case == "init":
        ap, an = (float(torch.log(torch.expm1(torch.tensor(v, dtype=dtype)))) for v in (0.8, 0.8 - 0.5))
    return torch.tensor([ap], dtype=dtype, device=device), torch.tensor([an], dtype=dtype, device=device)


# ---- fp64 references ---------------------------------------------------------------------------------------------------------------
def sp64(a):
    return torch.where(a > 20, a, torch.log1p(torch.exp(torch.clamp(a, max=20.0))))


def sp_grad64(a):
    return torch.where(a > 20, torch.ones_like(a), torch.sigmoid(a))


def _scalars(ap_raw, an_raw, beta):
    """-> ap, an, and their fp32 errors in units of u32"""
    spp, spn = sp64(ap_raw.double().reshape(())), sp64(an_raw.double().reshape(()))
    ap, an = spp, beta + spn
    return ap, an, SP * spp, SP * spn + an.abs()


def _em(x64, eps):
    xm = torch.minimum(x64, torch.full_like(x64, eps))
    xm = torch.where(x64 > 0, torch.zeros_like(xm), xm)           # unused on the positive branch
    em = torch.expm1(xm)
    return xm, em, EM * em.abs() + 2.0 * xm.abs() * torch.exp(xm)


def fwd_reference(x, ap_raw, an_raw, beta, eps):
    """-> (y, E) [u of x's dtype]"""
    x64 = x.double()
    ap, an, e_ap, e_an = _scalars(ap_raw, an_raw, beta)
    xm, em, e_em = _em(x64, eps)
    pos = x64 > 0
    d = em - x64
    y = torch.where(pos, ap * x64 * x64 + beta * x64, an * d + beta * x64)
    f_pos = (e_ap + 2.0 * ap) * x64 * x64 + 2.0 * (beta * x64).abs()
    f_neg = an.abs() * (e_em + d.abs()) + e_an * d.abs() + (beta * x64).abs() + y.abs()
    F = torch.where(pos, f_pos, f_neg)
    return y, _units(y, F, x.dtype)


def _units(ref, F, dtype):
    """E in units of the output's u from the value (one rounding to bf16) and the fp32 terms F, with the underflow floor"""
    F = F + 4.0 * FLOOR
    return (ref.abs() + FLOOR + _uscale(dtype) * F) if dtype == BF else F


def _bwd_parts(x, dy, ap_raw, an_raw, beta, eps):
    x64, dy64 = x.double(), dy.double()
    ap, an, e_ap, e_an = _scalars(ap_raw, an_raw, beta)
    xm, em, e_em = _em(x64, eps)
    pos = x64 > 0
    m = torch.where(x64 < eps, 1.0, torch.where(x64 == eps, 0.5, 0.0)).to(torch.float64)
    ge = m * torch.exp(xm) - 1.0
    g = torch.where(pos, 2.0 * ap * x64 + beta, an * ge + beta)
    f_g = torch.where(pos, 2.0 * e_ap * x64.abs() + (2.0 * ap * x64).abs() + abs(beta),
                      an.abs() * (m * e_em + ge.abs()) + e_an * ge.abs() + (an * ge).abs() + abs(beta))
    dx = dy64 * g
    F_dx = dy64.abs() * f_g + dx.abs()
    d = em - x64
    tp = torch.where(pos, dy64 * x64 * x64, torch.zeros_like(x64))
    tn = torch.where(pos, torch.zeros_like(x64), dy64 * d)
    f_tp = 2.0 * tp.abs()
    f_tn = torch.where(pos, torch.zeros_like(x64), dy64.abs() * (e_em + d.abs()) + tn.abs())
    return dx, F_dx, tp, f_tp, tn, f_tn


def bwd_reference(x, dy, ap_raw, an_raw, beta, eps):
    """-> (dx, E_dx)"""
    dx, F, *_ = _bwd_parts(x, dy, ap_raw, an_raw, beta, eps)
    return dx, _units(dx, F, x.dtype)


def dalpha_reference(x, dy, ap_raw, an_raw, beta, eps, old_p=None, old_n=None):
    """-> ((dalpha_p, E), (dalpha_n, E)) [u of the dtype]; old_*: the stored values an accumulating launch adds to (else None)"""
    _, _, tp, f_tp, tn, f_tn = _bwd_parts(x, dy, ap_raw, an_raw, beta, eps)
    dep = depth(x.numel())
    out = []
    for raw, t, f, old in ((ap_raw, tp, f_tp, old_p), (an_raw, tn, f_tn, old_n)):
        s = sp_grad64(raw.double().reshape(()))
        S = t.sum()
        F_S = f.sum() + dep * t.abs().sum() + 4.0 * FLOOR * x.numel()
        ref = s * S
        F = s * F_S + (SP + 1.0) * ref.abs()
        if old is not None:
            ref = ref + old.double().reshape(())
            F = F + ref.abs()
        E = _units(ref, F, x.dtype)
        out.append((ref.reshape(1), E.reshape(1)))
    return out


# ---- the fp32 emulation of the documented operation order (CPU) --------------------------------------------------------------------
def _f(t):
    return t.to(torch.float32)


def _fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in fp64, the sum rounds once there and once more to fp32"""
    return (a.double() * b.double() + c.double()).float()


def _sp32(a):
    a = _f(a)
    return torch.where(a > 20, a, torch.log1p(torch.exp(torch.clamp(a, max=20.0))))


def _sp_grad32(a):
    a = _f(a)
    return torch.where(a > 20, torch.ones_like(a), 1.0 / (1.0 + torch.exp(-a)))


def _expm1_neg32(x):
    q = torch.full_like(x, 1.0 / 5040.0)
    for c in (1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5):
        q = _fma(q, x, torch.full_like(x, c))
    small = _fma(x * x, q, x)
    big = torch.exp(x) - 1.0
    return torch.where(x > -0.35, small, big)


def emulate_fwd(x, ap_raw, an_raw, beta, eps):
    xf = _f(x.cpu())
    ap, an = _sp32(ap_raw.cpu()).reshape(()), (beta + _sp32(an_raw.cpu())).reshape(())
    b = torch.tensor(beta, dtype=torch.float32)
    pos = _fma(ap.expand_as(xf), xf, b.expand_as(xf)) * xf
    em = _expm1_neg32(torch.minimum(torch.minimum(xf, torch.tensor(eps, dtype=torch.float32)), torch.zeros_like(xf)))
    neg = _fma(an.expand_as(xf), em - xf, b * xf)
    return torch.where(xf > 0, pos, neg).to(x.dtype)


def _tree256(v):
    """block_sum_256 of v [..., 256]: the xor-shuffle butterfly inside each of the 4 waves, then ((r0 + r1) + r2) + r3"""
    w = v.reshape(*v.shape[:-1], 4, 64)
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., idx ^ o]
    r = w[..., 0]
    return ((r[..., 0] + r[..., 1]) + r[..., 2]) + r[..., 3]


def emulate_bwd(x, dy, ap_raw, an_raw, beta, eps, old_p=None, old_n=None):
    """-> (dx in T, dalpha_p in T [1], dalpha_n in T [1]): the kernels' arithmetic and summation order in fp32 on the CPU"""
    dtype, n = x.dtype, x.numel()
    xf, df = _f(x.cpu()), _f(dy.cpu())
    ap, an = _sp32(ap_raw.cpu()).reshape(()), (beta + _sp32(an_raw.cpu())).reshape(())
    b, e = torch.tensor(beta, dtype=torch.float32), torch.tensor(eps, dtype=torch.float32)
    em = _expm1_neg32(torch.minimum(torch.minimum(xf, e), torch.zeros_like(xf)))
    ge = torch.where(xf < e, em, torch.where(xf == e, _fma(torch.full_like(em, 0.5), em, torch.full_like(em, -0.5)), torch.full_like(em, -1.0)))
    pos = xf > 0
    g = torch.where(pos, _fma((ap + ap).expand_as(xf), xf, b.expand_as(xf)), _fma(an.expand_as(xf), ge, b.expand_as(xf)))
    dx = (df * g).to(dtype)
    tp = torch.where(pos, df * xf * xf, torch.zeros_like(xf))
    tn = torch.where(pos, torch.zeros_like(xf), df * (em - xf))
    it, nb, vn = iters(n), blocks(n), VN[dtype]
    vpl = WG_ELEMS // 256 // vn
    out = []
    for t, raw, old in ((tp, ap_raw, old_p), (tn, an_raw, old_n)):
        pad = torch.zeros(nb * it * WG_ELEMS, dtype=torch.float32)
        pad[:n] = t
        lanes = pad.reshape(nb, it * vpl, 256, vn)                 # element (pass, lane, k) of a workgroup's run
        acc = torch.zeros(nb, 256, dtype=torch.float32)
        for p in range(it * vpl):
            for k in range(vn):
                acc = acc + lanes[:, p, :, k]
        part = _tree256(acc)                                       # [nb]
        rounds = -(-nb // 256)
        pp = torch.zeros(rounds * 256, dtype=torch.float32)
        pp[:nb] = part
        pp = pp.reshape(rounds, 256)
        acc = torch.zeros(256, dtype=torch.float32)
        for r in range(rounds):
            acc = acc + pp[r]
        gsum = _sp_grad32(raw.cpu()).reshape(()) * _tree256(acc)
        if old is not None:
            gsum = gsum + _f(old.cpu()).reshape(())
        out.append(gsum.reshape(1).to(dtype))
    return dx, out[0], out[1]


# ---- the contract test's inputs (shared with the CPU emulation that fixed the constants) -------------------------------------------
NS = (1, 7, 8, 9, 2047, 2048, 2049, 16 * 264, 300001)       # the vector tail, exactly one workgroup, one element past it, 147 workgroups
N_REDUCE_PASSES = 2048 * 600 + 5                           # 601 workgroups: the finishing launch's lanes add 3 partials each
N_ITERS2 = WG_ELEMS * MAX_BLOCKS + 2049                    # past XIELU_MAX_BLOCKS runs: a workgroup takes two passes
SCALES = (1e-3, 1.0, 30.0)


def contract_cases(n):
    """(scale, alpha case, accumulate) combinations run at size n: all 18 up to 300001, one at the two large sizes"""
    if n > 300001:
        return [(1.0, "init", n == N_REDUCE_PASSES)]
    return [(s, a, acc) for s in SCALES for a in ALPHA_CASES for acc in (False, True)]


def old_values(dtype, device):
    """what an accumulating launch finds in the gradients' storage"""
    return torch.tensor([0.75], dtype=dtype, device=device), torch.tensor([-1.5], dtype=dtype, device=device)
