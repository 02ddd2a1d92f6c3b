"""Optimizer kernel checker (csrc/mm_optim.hip): fp64 references with per-element error scales for single calls, and pure
integer references for the (bf16 parameter, 16-bit remainder) form of the fp32 master.

Every reference reads the STORED operands the kernel reads -- g, m, v, master or join(p, lo) as device bits, clip[1] as the fp32
value mm_gradnorm_finish stored, the hyper-parameters after conversion to fp32 (`f32`) -- and returns fp64 (ref, E) for the rule of
tests/kernel_check.py.  E is in units of U32 for every output here (all are fp32, or exact functions of an fp32 value).  A run of
several steps feeds the kernel's own outputs back as the next inputs, so every step is judged alone.

Sum of squares (sumsq_kernel, gradnorm_finish_kernel).  Vector j of 16 bytes goes to block (j / 256) % nblk, thread j % 256; the
scalar tail [VN (n / VN), n) goes to block 0.  partial[b] = fp64 sum of its g^2, E = that sum * (1 + depth): one rounding for the
square and `sumsq_depth` additions on the longest path (a thread's strided adds, + 1 for the tail, + 6 shuffle levels + 3 adds
of the four wave sums).  A block with no work writes exactly 0 (E = 0).  total[0] = sqrtf(sum partial): half the relative error
of the sum (`finish_depth`: the 256-strided adds and the same tree) + 1 for the root.  total[1] is judged from the kernel's OWN
total[0]: min(1, max_norm / (nrm + 1e-6f)) with one rounding each for the add and the divide; exactly 1.0 where max_norm <= 0 and
where the unclamped quotient exceeds 1 by more than its error.  `sumsq_exact_problem` makes every partial sum an integer below 2^24
quanta, exact in any order: partial and total[0] must then equal the reference bit for bit.

AdamW, one step (adamw_kernel, adamw_split_kernel), one term per fp32 rounding point, carried through the derivative:
  gc = g c                 1 rounding (none where c == 1)
  m' = b1 m + (1-b1) gc    two products, the add, the carried error of gc           [(1 - b) is exact in fp32 for b >= 0.5]
  v' = b2 v + (1-b2) gc gc three products, the add, twice the relative error of gc
  wd' = w (1 - lr wd)      lr wd, 1 - x, the multiply
  upd = lr (m' / bc1) / (sqrt(v' / bc2) + eps)
                           relative to |upd|: m', / bc1, * lr, the final /, and in the denominator v' and / bc2 (both halved
                           through the root), the root's own rounding and the + eps, each scaled by its share of sqrt + eps
  w' = wd' - upd           the subtract
The compiler may contract a multiply-add; that only removes roundings, so the bound stays valid -- and bit equality with a torch
fp32 replay of this arithmetic is never asserted.

Bias correction.  mm_adamw_step* evaluate bc = 1.0f - powf(beta, (float) step) in fp32; the references evaluate it in fp64 from
the fp32 beta.  With beta2 = 0.999f the fp32 value is off from the fp64 one by -112 u32 (relative) at step 2, +105 u32 at step 3,
-5.5 u32 at step 10, and exact at step 1 and from about step 1000: an error of the power (at most half an ulp for a correctly
rounded powf) is amplified by beta^step / bc, 499 at step 2.  E carries 1 u32 of beta^step -- the 0.5 of a correctly rounded powf,
doubled -- times that amplification, plus the rounding of the subtraction where beta^step < 0.5; half of bc2's term reaches the
update.  numpy's float32 `power` does not always equal libm powf (0.95, step 10 differs), so recomputing bc "in fp32" on the host
would be wrong in both directions.

Exact parts: p == RNE_bf16(master_out) (bf16) or p == master_out (fp32) bit for bit; for the split entry join(p, lo) is held to
w' and (p, lo) must be a fixed point of the integer split.  The integer reference: p = RNE(w), d = bits(w) - (bits(p) << 16) in
[-0x8000, 0x8000], lo = min(d, 32767), join = (bits(p) << 16) + sign-extended lo.  d = +0x8000 (low half 0x8000 under an even upper
half: a tie rounded down) is the only lossy case; it is stored as 0x7FFF, one fp32 ulp below, and E gets one ulp of |w'| exactly
where lo == 0x7FFF.

c per output is in `C`: the smallest power of two >= 2x the worst err / (u E) measured on the MI355X over
tests/test_optim_contract_gpu.py (MM_OPTIM_RATIO_LOG writes the ratios); E is a worst case, so no c exceeds 2."""
import ctypes

import torch

from tests.kernel_check import U32, RatioLog, check_bits, check_bound

BF, F32 = torch.bfloat16, torch.float32
VN = {BF: 8, F32: 4}
NAME = {BF: "bf16", F32: "f32"}
OK, ERR_ARG, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -3
RATIOS = RatioLog("MM_OPTIM_RATIO_LOG")

# c per output: the smallest power of two >= 2x the worst err / (u E) measured on the MI355X over
# tests/test_optim_contract_gpu.py; the measured ratio in the comment
C = {
    "optim.sumsq": 0.5,     # 0.134
    "optim.norm": 0.5,      # 0.154
    "optim.coef": 1.0,      # 0.464 (0.474 with tests/test_kernels_gpu.py)
    "optim.m": 2.0,         # 0.846
    "optim.v": 2.0,         # 0.763
    "optim.master": 2.0,    # 0.987: where the update is small, the one rounding of the subtract at a value just above a power of two
    "optim.split": 2.0,     # 0.987 (the same element through join(p, lo))
}                           # "optim.p" needs none: the parameter is an exact function of the master and is compared bit for bit
PREFIX = [""]               # tests/test_optim_check_cpu.py records its emulations under "emulation." instead


def bound(name, key, got, ref, E):
    return check_bound(name, got, ref.to(got.device), E.to(got.device), C[key], U32, key=PREFIX[0] + key, log=RATIOS)


def f32(x):
    """the value a C float argument takes"""
    return ctypes.c_float(x).value


def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


# ---- sum of squares ------------------------------------------------------------------------------------------------------------
def block_of(n, nblk, dtype, device="cpu"):
    """the block that adds element i of the gradient: [n] int64"""
    vn = VN[dtype]
    i = torch.arange(n, device=device)
    b = (i // vn // 256) % nblk
    b[n // vn * vn:] = 0
    return b


def sumsq_depth(n, nblk, dtype):
    vn = VN[dtype]
    per_thread = -(-(n // vn) // (nblk * 256)) * vn
    return per_thread + 1 + 6 + 3


def finish_depth(nblk):
    return -(-nblk // 256) + 6 + 3


def sumsq_bodies(n, nblk, dtype):
    """which loops of sumsq_kernel thread 0 of block 0 runs: a subset of {'unrolled', 'single', 'tail'}"""
    vn = VN[dtype]
    nv, st, i, out = n // vn, nblk * 256, 0, set()
    while i + 3 * st < nv:
        out.add("unrolled")
        i += 4 * st
    if i < nv:
        out.add("single")
    if n % vn:
        out.add("tail")
    return out


def sumsq_problem(n, dtype, device, seed):
    """gradients over four decades so that no block's sum looks like another's"""
    g = _gen(device, seed)
    x = torch.randn(n, generator=g, device=device) * torch.exp2(torch.randint(-6, 7, (n,), generator=g, device=device).float())
    return x.to(dtype)


def sumsq_exact_problem(n, dtype, device, seed, amp=7, shift=-5):
    """small integers times one power of two -> (g, quantum of g^2)"""
    g = torch.randint(-amp, amp + 1, (n,), generator=_gen(device, seed), device=device).double() * 2.0 ** shift
    return g.to(dtype), 4.0 ** shift


def partial_reference(g, nblk):
    """-> (partial [nblk], E [U32])"""
    n, g2 = g.numel(), g.double() ** 2
    ref = torch.zeros(nblk, dtype=torch.float64, device=g.device).index_add_(0, block_of(n, nblk, g.dtype, g.device), g2)
    return ref, ref * (1 + sumsq_depth(n, nblk, g.dtype))


def assert_exact_range(g, quantum):
    worst = float((g.double() ** 2).sum()) / quantum
    assert worst < 2.0 ** 24, f"exact family out of range: sum g^2 / quantum reaches {worst:.4g} >= 2^24"


def norm_reference(partial):
    """total[0] from the stored partials -> (nrm, E [U32])"""
    s = partial.double().sum()
    nrm = s.sqrt().reshape(1)
    return nrm, nrm * (0.5 * finish_depth(partial.numel()) + 1)


def gradnorm_reference(g, nblk_each, nblk_total=None):
    """total[0] end to end from the gradient (one tensor) -> (nrm, E [U32])"""
    nrm = (g.double() ** 2).sum().sqrt().reshape(1)
    d = 1 + sumsq_depth(g.numel(), nblk_each, g.dtype) + finish_depth(nblk_total or nblk_each)
    return nrm, nrm * (0.5 * d + 1)


def coef_reference(nrm_f32, max_norm):
    """total[1] from the kernel's own total[0] (a python float holding the fp32 value) -> (coef, E [U32]) as [1] tensors"""
    mx = f32(max_norm)
    if not mx > 0:
        return torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    q = mx / (nrm_f32 + f32(1e-6))
    E = 2.0 * q
    if q - 1 > C["optim.coef"] * U32 * E:
        return torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    return torch.tensor([min(1.0, q)], dtype=torch.float64), torch.tensor([E], dtype=torch.float64)


def check_partial(tag, g, nblk, partial, exact_quantum=None):
    ref, E = partial_reference(g, nblk)
    if exact_quantum is not None:
        assert_exact_range(g, exact_quantum)
        check_bits(tag + " partial (exact family)", partial, ref.float())
    return bound(tag + " partial", "optim.sumsq", partial, ref, E)


def check_total(tag, partial, max_norm, total, g=None, nblk_each=None, exact=False):
    """total [2] against the stored partials (and end to end against g when given)"""
    ref, E = norm_reference(partial)
    bound(tag + " total[0] from the partials", "optim.norm", total[:1], ref, E)
    if g is not None:
        ref, E = gradnorm_reference(g, nblk_each, partial.numel())
        bound(tag + " total[0] from the gradient", "optim.norm", total[:1], ref, E)
        if exact:
            check_bits(tag + " total[0] (exact family)", total[:1], ref.float())
    cref, cE = coef_reference(float(total[0]), max_norm)
    assert float(total[1]) <= 1.0, f"{tag}: clip coefficient {float(total[1])} > 1"
    bound(tag + " total[1]", "optim.coef", total[1:].cpu(), cref, cE)


def check_gradnorm(tag, g, nblk, max_norm, total):
    """kernels.gradnorm on one tensor, end to end: total[0] against the gradient, total[1] from total[0]"""
    ref, E = gradnorm_reference(g, nblk)
    bound(tag + " total[0]", "optim.norm", total[:1], ref, E)
    cref, cE = coef_reference(float(total[0]), max_norm)
    bound(tag + " total[1]", "optim.coef", total[1:].cpu(), cref, cE)


# ---- AdamW ---------------------------------------------------------------------------------------------------------------------
class Hyper:
    """the fp32 values the entry receives"""

    def __init__(self, lr, b1, b2, eps, wd):
        self.lr, self.b1, self.b2, self.eps, self.wd = (f32(x) for x in (lr, b1, b2, eps, wd))

    def args(self):
        return tuple(ctypes.c_float(x) for x in (self.lr, self.b1, self.b2, self.eps, self.wd))


def _one_minus(b):
    """fp64 (1 - b) and the relative error [U32] of the kernel's fp32 `1.f - b`"""
    x = 1.0 - b
    x32 = float(torch.tensor(1.0, dtype=F32) - torch.tensor(b, dtype=F32))
    return x, abs(x32 - x) / x / U32


def bias_correction(beta, step):
    """fp64 bc = 1 - beta^step from the fp32 beta, and the relative error [U32] allowed for the fp32 evaluation"""
    pw = beta ** step
    bc = 1.0 - pw
    return bc, pw / bc + (0.0 if pw >= 0.5 else 1.0)


def adamw_reference(g, m, v, w, h, step, c=1.0):
    """one step from the stored operands (g in its dtype, m, v, w fp32; c the fp32 clip coefficient or 1.0)
    -> dict name -> (ref, E [U32]) for m, v, w."""
    g64, m64, v64, w64 = g.double(), m.double(), v.double(), w.double()
    gc = g64 * c
    e_gc = gc.abs() * (0.0 if c == 1.0 else 1.0)
    o1, r1 = _one_minus(h.b1)
    o2, r2 = _one_minus(h.b2)
    mo = h.b1 * m64 + o1 * gc
    E_m = (h.b1 * m64).abs() + (o1 * gc).abs() * (1 + r1) + mo.abs() + o1 * e_gc
    vo = h.b2 * v64 + o2 * gc * gc
    E_v = (h.b2 * v64).abs() + (o2 * gc * gc) * (2 + r2) + vo.abs() + o2 * 2 * gc.abs() * e_gc
    d = 1.0 - h.lr * h.wd
    wd_ = w64 * d
    E_wd = w64.abs() * (h.lr * h.wd + (2 * d if h.wd != 0 else 0.0))      # wd == 0: 1 - 0 and w * 1 are exact
    bc1, e1 = bias_correction(h.b1, step)
    bc2, e2 = bias_correction(h.b2, step)
    r = (vo / bc2).sqrt()
    den = r + h.eps
    upd = h.lr * (mo / bc1) / den
    rel_v = torch.where(vo > 0, E_v / torch.where(vo > 0, vo, torch.ones_like(vo)), torch.zeros_like(vo))
    rel_den = (0.5 * (rel_v + 1 + e2) + 1) * (r / den) + 1
    E_upd = upd.abs() * (3 + e1 + rel_den) + (h.lr / bc1) / den * E_m
    wo = wd_ - upd
    E_w = E_wd + E_upd + wo.abs()
    return {"m": (mo, E_m), "v": (vo, E_v), "w": (wo, E_w)}


def adamw_problem(n, dtype, device, seed, gscale=1.0):
    """g, m random, v >= 0 random, master over three decades, with planted blocks (each `k` = min(n // 8, 64) elements, from the
    front): master = 0; g = 0; g = m = v = 0.  -> dict of g [dtype], m, v, w [fp32] and the block length k."""
    gen = _gen(device, seed)
    rn = lambda: torch.randn(n, generator=gen, device=device)
    g = (rn() * gscale).to(dtype)
    m = rn() * gscale * 0.3
    v = (rn() * gscale * 0.5) ** 2
    w = rn() * torch.exp2(torch.randint(-4, 3, (n,), generator=gen, device=device).float())
    k = min(n // 8, 64)
    w[:k] = 0
    g[k:2 * k] = 0
    g[2 * k:3 * k] = 0
    m[2 * k:3 * k] = 0
    v[2 * k:3 * k] = 0
    return {"g": g, "m": m, "v": v, "w": w, "k": k}


def plant_ties(p, lo, start, count):
    """(p, lo) whose join has the low half 0x8000 under an EVEN upper half: an odd p with lo = -0x8000.  No split produces that
    pair, but join accepts it, and the split of its value is the lossy case (d = +0x8000, stored as 0x7FFF)."""
    sl = slice(start, start + count)
    pi = p.view(torch.int16)
    pi[sl] = pi[sl] | 1
    lo[sl] = -32768


def check_adamw(tag, before, after, h, step, c=1.0, kind="bf16"):
    """before: g, m, v, w (the fp32 master the kernel read: `master` or join(p, lo)); after: m, v and, per kind,
    'bf16' / 'f32': master, p;  'split': p, lo.  Returns nothing; raises on the first violation."""
    ref = adamw_reference(before["g"], before["m"], before["v"], before["w"], h, step, c)
    bound(tag + " m", "optim.m", after["m"], *ref["m"])
    bound(tag + " v", "optim.v", after["v"], *ref["v"])
    w64, E_w = ref["w"]
    if kind == "split":
        p, lo = after["p"], after["lo"]
        w = join_reference(p, lo)
        E_w = E_w + 2.0 * w64.abs() * (lo == 0x7FFF).to(E_w.device)
        bound(tag + " join(p, lo)", "optim.split", w, w64, E_w)
        p2, lo2 = split_reference(w)
        check_bits(tag + " p is RNE(join(p, lo))", p, p2)
        assert bool((lo == lo2).all()), f"{tag}: lo is not the remainder of join(p, lo)"
    else:
        bound(tag + " master", "optim.master", after["master"], w64, E_w)
        check_bits(tag + " p = T(master)", after["p"], rne_bf16(after["master"]) if kind == "bf16" else after["master"])
    if h.wd == 0:       # g = m = v = 0 without decay: w * 1 - 0 / eps is w itself, whatever the compiler contracts
        still = ((ref["m"][0] == 0) & (ref["v"][0] == 0)).to(before["w"].device)
        if kind == "split":
            p0, lo0 = split_reference(before["w"])
            check_bits(tag + " p where nothing moves", after["p"][still], p0[still])
            assert bool((after["lo"][still] == lo0[still]).all()), f"{tag}: lo changed where nothing moves (or +0x8000 is not stored as 0x7FFF)"
        else:
            check_bits(tag + " master where nothing moves", after["master"][still], before["w"][still])


# ---- the integer split ---------------------------------------------------------------------------------------------------------
def _bits(w):
    return w.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def rne_bf16(w):
    """round to nearest even on the bits (no NaN) -> bf16"""
    b = _bits(w)
    p = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    return _as_i16(p).view(BF)


def _as_i16(x):
    return torch.where(x >= 0x8000, x - 0x10000, x).to(torch.int16)


def split_reference(w):
    """fp32 -> (p bf16, lo int16)"""
    b = _bits(w)
    p = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    d = b - (p << 16)
    return _as_i16(p).view(BF), torch.clamp(d, max=32767).to(torch.int16)


def join_reference(p, lo):
    """(p bf16, lo int16) -> fp32"""
    b = ((p.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF) << 16) + lo.to(torch.int64)
    b = b & 0xFFFFFFFF
    return torch.where(b >= 0x80000000, b - 0x100000000, b).to(torch.int32).view(F32)


LOW_HALVES = [0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF]
UPPER_HALVES = {                    # (even, odd) upper halves of the positive value
    "zero / denormal": (0x0000, 0x0001),
    "denormal, mantissa carry": (0x007E, 0x007F),
    "1.0": (0x3F80, 0x3F81),
    "mantissa all ones": (0x3FFE, 0x3FFF),
    "rounds to infinity": (0x7F7E, 0x7F7F),
}


def constructed_bits(device):
    """every combination of low half x upper half (even, odd) x sign, then +-infinity -> (w fp32, lossy bool): lossy marks the
    elements where join(split(w)) is one ulp below w (low half 0x8000 under an even upper half)."""
    vals, lossy = [], []
    for ev, od in UPPER_HALVES.values():
        for hi in (ev, od):
            for low in LOW_HALVES:
                for sign in (0, 0x8000):
                    vals.append(((hi | sign) << 16) | low)
                    lossy.append(low == 0x8000 and hi % 2 == 0)
    for inf in (0x7F800000, 0xFF800000):
        vals.append(inf)
        lossy.append(False)
    b = torch.tensor(vals, dtype=torch.int64, device=device)
    w = torch.where(b >= 0x80000000, b - 0x100000000, b).to(torch.int32).view(F32)
    return w, torch.tensor(lossy, device=device)


def tiled(t, n):
    """t repeated to n elements"""
    return t.repeat(-(-n // t.numel()))[:n].contiguous()


def ulp_below(w):
    """the fp32 value one step towards zero in magnitude: bits - 1"""
    return (w.contiguous().view(torch.int32) - 1).view(F32)
