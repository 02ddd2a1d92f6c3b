"""Row-wise kernel checker (csrc/mm_rowwise.hip): fp64 references with per-element error scales, asymmetric problems, guarded launches.

Every reference takes the STORED operands (bf16 / fp32 tensors, any device) and returns (ref, E) in fp64 for the rule of
tests/kernel_check.py (`bound`).  The rounding points, read off mm_rowwise.hip (T = storage type, everything else fp32):

  rmsnorm_fwd   ss = sum x^2 (depth norm_depth) -> ss / H -> + eps -> rsqrtf = rstd;  y = T(w * f32(T(x * rstd))): two roundings to T
  rmsnorm_bwd   xh = x rstd;  dot = sum(g w xh) / H (norm_depth);  dx = T(rstd (g w - xh dot) + dres);  dw = reduce(sum_rows g xh)
  layernorm_fwd mu = sum x / H;  var = sum (x - mu)^2 / H;  rstd = rsqrtf(var + eps);  y = T((x - mu) rstd w + b): one rounding to T
  layernorm_bwd s1 = sum(g w) / H, s2 = sum(g w xh) / H;  dx = T(rstd (g w - s1 - xh s2) + dres);  dw, db = reduce(row sums)
  rope_table    ang = f32(pos) * inv_freq (ONE fp32 product: the documented angle), cosf / sinf, optionally rounded to bf16
  rope_apply    lo' = fma(lo, c, -(hi s)), hi' = fma(hi, c, lo s): a product and an fma, then T
  swiglu_fwd    T(f32(T(g / (1 + exp(-g)))) * u);  swiglu_bwd: one rounding to T per output
  gelu          one rounding to T;  the function's fp32 evaluation error is FUNC-style (a few ulps of x and of f(x))
  ce_fwd        per-thread online (max, sum) over ce_iters(V) vectors, block max, rescale, block sum, lse = max + logf(sum)
  ce_bwd        T((exp(x - lse) - [v == label]) * gscale / max(count, 1))
  argmax        s = f32(T(x / temp)), p = T(exp(s - max s) / sum), first index of the maximum of p
  expert_fuse   w = gate[n, idx[j]] (mode 1: their J-way softmax in fp32);  T(sum_j w_j x_j) / T(w'_j x_j): one rounding to T
                (c derived, not measured: see the section at the end)

Summation depth.  The accumulation term of a reduction is (depth) * u32 * sum|terms| with the kernel's real worst-case depth:
  norm_depth(dtype, H) = CH_body * VN products added by one thread + 6 shuffle levels + 3 adds of the 4 wave sums (block_sum_256),
      CH_body the instantiated chunk count (1, 2, 4, 8) -- at most 73 for bf16 and 41 for fp32, whatever H;
  reduce_depth(nblk)   = ceil(nblk / 256) adds per accumulator of the unrolled body + 3 of the 64-stride tail + 2 to join the four
      accumulators + 6 LDS tree levels + 1 for `accumulate`;
  dw / db              = 16 rows per block (NORM_BWD_ROWS_PER_BLOCK) + 2 for the products + reduce_depth(nblk);
  ce_depth(dtype, V)   = ce_iters * (VN + 1) + 9;   ce_reduce: ceil(T / 256) + 9.

c per kernel is in `C`: the smallest power of two >= 2x the worst err / (u E) measured on the MI355X over
tests/test_rowwise_contract_gpu.py and the older row-wise tests (MM_GEMM_RATIO_LOG writes the ratios, paths
`rowwise.<kernel>.<dtype>`).  The depths are worst cases and rounding errors do not line up, so the fp32 statistics of a correct
kernel measure well below 1; a bf16 output measures just under 1 (half an ulp of a value just above a power of two is u)."""
import torch

from tests import gemm_check as GC
from tests.gemm_check import FUNC, RATIOS, check_exact, pad64  # noqa: F401  (the row-wise ratios go into the GEMM log)
from tests.kernel_check import U, U32, Guarded, check_bound, sentinel_fill

BF, F32 = torch.bfloat16, torch.float32
U_BF = U[BF]
VN = {BF: 8, F32: 4}
NAME = {BF: "bf16", F32: "f32"}
ROWS_PER_BLOCK = 16                  # NORM_BWD_ROWS_PER_BLOCK
ARGMAX_CHUNK = 4096
OK, ERR_ARG, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -3

# c per path (bf16, f32): the smallest power of two >= 2x the worst err / (u E) measured on the MI355X over
# tests/test_rowwise_contract_gpu.py and the older row-wise tests; the measured ratios (bf16, f32) in the comment
C = {
    "rmsnorm.rstd": (0.5, 0.5),        # 0.210, 0.215
    "rmsnorm.y": (2.0, 1.0),           # 0.986, 0.290
    "rmsnorm.dx": (2.0, 1.0),          # 0.996, 0.477
    "rmsnorm.dw": (2.0, 0.5),          # 0.995, 0.135
    "layernorm.mean": (0.25, 0.5),     # 0.065, 0.183
    "layernorm.rstd": (0.5, 0.5),      # 0.175, 0.200
    "layernorm.y": (2.0, 0.5),         # 0.996, 0.196
    "layernorm.dx": (2.0, 1.0),        # 0.996, 0.360
    "layernorm.dw": (2.0, 0.5),        # 0.995, 0.135
    "layernorm.db": (2.0, 0.25),       # 0.995, 0.100
    "rope_table": (2.0, 2.0),          # 0.978 (tables rounded to bf16), 0.532 (fp32 tables)
    "rope": (2.0, 2.0),                # 0.995, 0.507
    "swiglu_fwd": (2.0, 0.25),         # 0.971, 0.082
    "swiglu_bwd": (2.0, 0.5),          # 0.996, 0.179
    "gelu_fwd": (2.0, 0.25),           # 0.995, 0.089
    "gelu_bwd": (2.0, 1.0),            # 0.986, 0.331
    "ce.lse": (0.25, 0.25),            # 0.110, 0.103
    "ce.loss_row": (0.25, 0.25),       # 0.091, 0.111
    "ce.loss": (0.125, 0.125),         # 0.051, 0.052
    "ce.dlogits": (2.0, 2.0),          # 0.995, 0.855
    # mm_expert_fuse, forward and backward = 1.  DERIVED, not measured: one output rounding bounds bf16 by 1, the fp32 terms are
    # counted explicitly in E (expert_fuse_reference), times 2 of margin.  The measured ratios are for the record only.
    "expert_fuse": (2.0, 2.0),         # 0.995, 0.416
}


def c_of(kernel, dtype):
    return C[kernel][0 if dtype == BF else 1]


PREFIX = ["rowwise"]                 # tests/test_rowwise_check_cpu.py records its emulation under "rowwise_emulation" instead


def path(kernel, dtype):
    return f"{PREFIX[0]}.{kernel}.{NAME[dtype]}"


def bound(name, kernel, dtype, got, ref, E, u=None):
    """The rule with the kernel's c, recorded under rowwise.<kernel>.<dtype>."""
    return check_bound(name, got, ref.to(got.device), E.to(got.device), c_of(kernel, dtype), U[dtype] if u is None else u,
                       key=path(kernel, dtype), log=RATIOS)


# ---- launch geometry mirrored from mm_rowwise.hip ------------------------------------------------------------------------------
def expected_ch(dtype, H):
    """norm_ch: chunks of 256 16-byte vectors a row needs; 1..8 are served, more is MM_ERR_UNSUPPORTED."""
    return -(-H // (256 * VN[dtype]))


def body_ch(dtype, H):
    """the DISPATCH_CH body that runs: ch 3 -> CH = 4, ch 5..7 -> CH = 8."""
    return {1: 1, 2: 2, 3: 4, 4: 4}.get(expected_ch(dtype, H), 8)


def norm_depth(dtype, H):
    return body_ch(dtype, H) * VN[dtype] + 6 + 3


def norm_blocks(M):
    return -(-M // ROWS_PER_BLOCK)


def reduce_depth(nblk):
    return -(-nblk // 256) + 3 + 2 + 6 + 1


def reduce_bodies(nblk):
    """which loops of reduce_partials_kernel row lane 0 runs: a subset of {'unrolled', 'tail'}."""
    b, out = 0, set()
    while b + 192 < nblk:
        out.add("unrolled")
        b += 256
    if b < nblk:
        out.add("tail")
    return out


def ce_iters(dtype, V):
    return -(-V // (256 * VN[dtype]))


def ce_depth(dtype, V):
    return ce_iters(dtype, V) * (VN[dtype] + 1) + 9


def _uscale(dtype):
    return U32 / U[dtype]


# ---- problems ----------------------------------------------------------------------------------------------------------------
def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def norm_problem(M, H, dtype, device, seed, layer=False):
    """x [M, H] with a per-row scale over 0.1 .. 20 (rstd differs row to row); w, b with a per-column ramp; LayerNorm rows carry
    a mean of 3 .. 7 times their spread, of either sign.  dy, dres random.  All in the storage dtype."""
    g = _gen(device, seed)
    r = lambda *s: torch.randn(*s, generator=g, device=device)
    u = lambda *s: torch.rand(*s, generator=g, device=device)
    scale = 0.1 * 200.0 ** u(M, 1)
    x = r(M, H) * scale
    if layer:
        x = x + scale * (3.0 + 4.0 * u(M, 1)) * torch.where(u(M, 1) < 0.5, -1.0, 1.0)
    ramp = torch.linspace(0.5, 1.5, H, device=device)
    w = ramp * (1.0 + 0.1 * r(H))
    b = (ramp - 1.0) * 2.0 + 0.1 * r(H)
    return {"x": x.to(dtype), "w": w.to(dtype), "b": b.to(dtype), "dy": r(M, H).to(dtype), "dres": r(M, H).to(dtype)}


def ce_problem(T, V, dtype, device, seed, scale=2.0):
    """logits [T, V] (normal, sigma = scale) whose row maximum is planted, row by row in turn, in the first vector, the last full
    vector and the ragged tail past V / VN * VN (the last column when there is none); labels cycle through 0, V - 1, the ragged
    tail, a random column and -100."""
    g = _gen(device, seed)
    x = torch.randn(T, V, generator=g, device=device) * scale
    vn = VN[dtype]
    Vv = V // vn * vn
    spots = [min(3, V - 1), max(0, Vv - 2), V - 1]
    labels = torch.randint(0, V, (T,), generator=g, device=device)
    for t in range(T):
        x[t, spots[t % 3]] = 4.0 * scale + 0.25 * (t % 5)
        labels[t] = (0, V - 1, Vv if V > Vv else V - 1, int(labels[t]), -100)[t % 5]
    return x.to(dtype), labels


def logits_storage(x, ld, extra_rows=4):
    """logits [T, V] in a [T + extra_rows, ld] storage with NaN sentinels in [V, ld) and in the rows past T -> the [T, V] view."""
    T, V = x.shape
    buf = sentinel_fill(torch.empty(T + extra_rows, ld, dtype=x.dtype, device=x.device))
    buf[:T, :V] = x
    return buf[:T, :V]


def rows_storage(x, extra_rows=4):
    """a contiguous [M, H] operand followed by rows of NaN sentinels (rows past M are not read)."""
    M, H = x.shape
    buf = sentinel_fill(torch.empty(M + extra_rows, H, dtype=x.dtype, device=x.device))
    buf[:M] = x
    return buf[:M]


def ld_vn(V, dtype):
    return -(-V // VN[dtype]) * VN[dtype]


# ---- RMSNorm -------------------------------------------------------------------------------------------------------------------
def rmsnorm_fwd_reference(x, w, eps):
    """-> (y, E_y [u of the dtype], rstd, E_rstd [U32]).  rstd's relative error in u32: half of (the sum's depth, the squares, / H,
    + eps) plus 2 for rsqrtf."""
    dtype, H = x.dtype, x.shape[1]
    x64, w64 = x.double(), w.double()
    rstd = torch.rsqrt((x64 * x64).mean(-1) + eps)
    y = x64 * rstd[:, None] * w64[None, :]
    e = 0.5 * (norm_depth(dtype, H) + 3) + 2.0
    # two roundings to T (T(x rstd), then the store), the fp32 product x * rstd, and rstd's own error
    return y, y.abs() * (2.0 + _uscale(dtype) * (e + 1.0)), rstd, rstd * e


def rmsnorm_chain(x, w, rstd):
    """The documented chain on the kernel's own rstd, in torch fp32: T(w * f32(T(x * rstd))).  Two separate multiplies, each
    rounded once: bit-exact whatever the device."""
    n = (x.float() * rstd.float()[:, None]).to(x.dtype).float()
    return (w.float()[None, :] * n).to(x.dtype)


def rmsnorm_bwd_reference(dy, x, w, rstd, dres=None):
    """rstd: the stored fp32 statistics the kernel reads.  -> (dx, E_dx, dw, E_dw), dw summed over all rows; E_dw in the units of a
    reduce_partials output of the same dtype."""
    dtype, (M, H) = x.dtype, x.shape
    g, x64, w64, rs = dy.double(), x.double(), w.double()[None, :], rstd.double()[:, None]
    xh = x64 * rs
    gw = g * w64
    dot, DOT = (gw * xh).mean(-1, keepdim=True), (gw * xh).abs().mean(-1, keepdim=True)
    dx = rs * (gw - xh * dot)
    d = norm_depth(dtype, H)
    Ef = 6.0 * rs * (gw.abs() + (xh * dot).abs()) + rs * xh.abs() * (d + 4) * DOT
    if dres is not None:
        dx = dx + dres.double()
        Ef = Ef + dres.double().abs()
    dw = (g * xh).sum(0)
    depth = ROWS_PER_BLOCK + 2 + reduce_depth(norm_blocks(M))
    return dx, dx.abs() + _uscale(dtype) * Ef, dw, dw.abs() + _uscale(dtype) * depth * (g * xh).abs().sum(0)


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------
def layernorm_fwd_reference(x, w, b, eps):
    """-> (y, E_y, mean, E_mean [U32], rstd, E_rstd [U32])."""
    dtype, H = x.dtype, x.shape[1]
    x64, w64, b64 = x.double(), w.double()[None, :], b.double()[None, :]
    d = norm_depth(dtype, H)
    mu = x64.mean(-1)
    E_mu = mu.abs() + (d + 1) * x64.abs().mean(-1)
    xc = x64 - mu[:, None]
    var = (xc * xc).mean(-1)
    rstd = torch.rsqrt(var + eps)
    # mean((x - mu')^2) = var + (mu' - mu)^2 exactly: the mean's error enters rstd in second order only
    e = 0.5 * (d + 5) + 2.0 + 0.5 * (E_mu * U32) ** 2 / (var + eps) / U32
    t = xc * rstd[:, None] * w64
    y = t + b64
    Ef = t.abs() * (e[:, None] + 4.0) + (E_mu * rstd)[:, None] * w64.abs() + b64.abs()
    return y, y.abs() + _uscale(dtype) * Ef, mu, E_mu, rstd, rstd * e


def layernorm_bwd_reference(dy, x, w, mean, rstd, dres=None):
    """mean / rstd: the stored fp32 statistics.  -> (dx, E_dx, dw, E_dw, db, E_db)."""
    dtype, (M, H) = x.dtype, x.shape
    g, w64, rs = dy.double(), w.double()[None, :], rstd.double()[:, None]
    xh = (x.double() - mean.double()[:, None]) * rs
    gw = g * w64
    s1, S1 = gw.mean(-1, keepdim=True), gw.abs().mean(-1, keepdim=True)
    s2, S2 = (gw * xh).mean(-1, keepdim=True), (gw * xh).abs().mean(-1, keepdim=True)
    dx = rs * (gw - s1 - xh * s2)
    d = norm_depth(dtype, H)
    Ef = 6.0 * rs * (gw.abs() + s1.abs() + (xh * s2).abs()) + rs * (d + 4) * (S1 + xh.abs() * S2)
    if dres is not None:
        dx = dx + dres.double()
        Ef = Ef + dres.double().abs()
    depth = ROWS_PER_BLOCK + 2 + reduce_depth(norm_blocks(M))
    dw, db = (g * xh).sum(0), g.sum(0)
    us = _uscale(dtype)
    return (dx, dx.abs() + us * Ef, dw, dw.abs() + us * depth * (g * xh).abs().sum(0), db, db.abs() + us * depth * g.abs().sum(0))


# ---- reduce_partials: the exact family -------------------------------------------------------------------------------------------
def partials_problem(nblk, H, device, seed, amp=64, span=3):
    """partials [nblk, H] f32 = small integers times a power of two per column; `before` [H] = what the output holds (integers in
    the column's quantum, representable in bf16).  -> (p, before, q)."""
    g = _gen(device, seed)
    q = torch.exp2(torch.randint(-span, span + 1, (H,), generator=g, device=device).double())
    p = torch.randint(-amp, amp + 1, (nblk, H), generator=g, device=device).double() * q[None, :]
    before = torch.randint(-amp, amp + 1, (H,), generator=g, device=device).double() * q
    return p.float(), before, q


def partials_reference(p, q, before=None):
    """fp64 sum of the partials (+ f32(out_before)) after asserting sum|p| / quantum < 2^24: every fp32 partial sum is then an
    integer multiple of the quantum below 2^24 quanta -- exact in any order -- and the output is ONE rounding of the result."""
    p64 = p.double()
    ref, mag = p64.sum(0), p64.abs().sum(0)
    if before is not None:
        ref, mag = ref + before.double(), mag + before.double().abs()
    worst = float((mag / q.double()).max()) if mag.numel() else 0.0
    assert worst < 2.0 ** 24, f"exact family out of range: sum|p| / q reaches {worst:.4g} >= 2^24"
    return ref


def rne(ref64, dtype):
    return ref64.float().to(dtype)


# ---- RoPE ----------------------------------------------------------------------------------------------------------------------
def rope_table_reference(pos, inv_freq, round_bf16):
    """fp64 cos / sin of the fp32 product float(pos) * inv_freq.  -> (cos, sin, E_cos, E_sin, u): cosf / sinf are held to 2 ulps of
    the result, and an ulp is up to 2 u32 of it: E = 4 |ref| (u = U32); with round_bf16 the one bf16 rounding is added (u = U_BF).
    (The first run measured 2.13 u32 = 1.1 ulp at cos(86 500 rad) = 1.0e-3, position 1 000 000.)"""
    ang = (pos.float()[:, None] * inv_freq.float()[None, :]).double()        # one fp32 rounding, as the kernel
    c, s = torch.cos(ang), torch.sin(ang)
    if round_bf16:
        k = 1.0 + 4.0 * U32 / U_BF
        return c, s, c.abs() * k, s.abs() * k, U_BF
    return c, s, 4.0 * c.abs(), 4.0 * s.abs(), U32


def rope_reference(x, cos, sin, nheads, D, inverse=False):
    """RoPE (inverse: sin -> -sin) on the first nheads * D columns of x [T, N]; the other columns pass unchanged.  Reuses
    gemm_check.rope_reference (E = |ref| + FUNC mag, bf16 units); for an fp32 output the arithmetic term is restated in fp32
    units: a product and an fma, 2 roundings of the magnitudes."""
    ref, E = GC.rope_reference(x.double(), cos, -sin if inverse else sin, nheads * D, D)
    if x.dtype == F32:
        E = ref.abs() + (E - ref.abs()) * (2.0 / FUNC)
    return ref, E


# ---- SwiGLU / GELU -------------------------------------------------------------------------------------------------------------
def _units(E, A, dtype):
    """gemm_check's references give E = A + FUNC B in bf16 units (FUNC = 16 U32 / U_BF): A + 16 B in fp32 units for an fp32 output."""
    return E if dtype == BF else A + (E - A) * (16.0 / FUNC)


def swiglu_fwd_reference(gu, I):
    ref, E = GC.swiglu_fwd_reference(gu[:, :I].double(), gu[:, I:2 * I].double())
    return ref, _units(E, 2.0 * ref.abs(), gu.dtype)


def swiglu_bwd_reference(gu, dout, I):
    """-> (dgu [M, 2I] = [dgate | dup], E)."""
    dg, E_dg, du, E_du = GC.swiglu_bwd_reference(gu[:, :I].double(), gu[:, I:2 * I].double(), dout.double())
    return torch.cat([dg, du], 1), torch.cat([_units(E_dg, dg.abs(), gu.dtype), _units(E_du, du.abs(), gu.dtype)], 1)


def swiglu_chain_check(name, gu, out, I):
    """bf16 forward, exactly: out = bf16(s * up) for s one of the two bf16 neighbours of silu(gate) (the product of two bf16
    values is exact in fp32, so that is one rounding).  The fp32 silu is a few ulps from the fp64 one and so rounds to one of
    them; a kernel that skips the intermediate rounding stores bf16(silu * up), which for many elements is neither."""
    assert gu.dtype == BF
    g, up = gu[:, :I], gu[:, I:2 * I]
    s64 = GC.silu64(g.double())
    near = s64.float().to(BF)
    bits = near.contiguous().view(torch.int16)
    step = torch.where(s64 > near.double(), 1, -1) * torch.where(near.double() < 0, -1, 1)
    other = torch.where((near == 0) | (s64 == near.double()), bits, bits + step.to(torch.int16)).view(BF)
    ok = torch.zeros_like(g, dtype=torch.bool)
    for s in (near, other):
        ok |= out.contiguous().view(torch.int16) == (s.float() * up.float()).to(BF).contiguous().view(torch.int16)
    if not bool(ok.all()):
        i = int((~ok).reshape(-1).nonzero()[0])
        raise AssertionError(f"{name}: {int((~ok).sum())} of {ok.numel()} elements are not bf16(bf16(silu(gate)) * up); first at "
                             f"(m={i // I}, n={i % I}): got {float(out.reshape(-1)[i])!r}")


GELU_KINDS = {0: "erf", 1: "quick", 2: "tanh"}


def gelu_fwd_reference(x, kind):
    ref, E = GC.act_reference(x.double(), GELU_KINDS[kind])
    return ref, _units(E, ref.abs(), x.dtype)


def gelu_bwd_reference(x, dy, kind):
    """dy * f'(x), f' by fp64 autograd of gemm_check.act64.  E = |ref| + FUNC |dy| (1 + |x|): f' is O(1) and is assembled from
    terms of size up to |x| (1 - tanh^2 times the inner derivative, x phi(x)) that cancel to fp32 absolute accuracy."""
    x64 = x.double().clone().requires_grad_(True)
    GC.act64(x64, GELU_KINDS[kind]).backward(dy.double())
    ref = x64.grad
    return ref, ref.abs() + (FUNC if x.dtype == BF else 16.0) * dy.double().abs() * (1.0 + x.double().abs())


def gelu_edge_values(dtype, device, n):
    """n values, normal (sigma 2), with |x| in {0, 1e-3, 5, 10, 30, 88} of both signs at the front and (n > 24) again at the end,
    where the scalar tail of an n that is not a multiple of VN handles them."""
    edge = torch.tensor([0.0, 1e-3, 5.0, 10.0, 30.0, 88.0], device=device)
    x = torch.randn(n, generator=_gen(device, n), device=device) * 2.0
    e = torch.cat([edge, -edge])
    k = min(n, e.numel())
    x[:k] = e[:k]
    if n > 24:
        x[n - 12:] = e
    return x.to(dtype)


# ---- cross entropy ---------------------------------------------------------------------------------------------------------------
def live_rows(labels, V):
    """rows that carry a loss and a gradient: 0 <= label < V."""
    return (labels >= 0) & (labels < V)


def counted_rows(labels):
    """rows mm_ce_reduce counts: label >= 0.  Callers only pass -100 or an in-range label, for which the two rules agree."""
    return labels >= 0


def ce_fwd_reference(logits, labels):
    """logits [T, V] (the valid columns), labels [T].  -> (lse, E_lse, loss_row, E_row) in U32 units.  A row needs one finite
    logit; -inf entries count as exp = 0."""
    dtype, (T, V) = logits.dtype, logits.shape
    x = logits.double()
    mx = x.max(-1).values
    lse = torch.logsumexp(x, -1)
    R = mx - torch.where(torch.isfinite(x), x, mx[:, None]).min(-1).values
    # relative error of the sum: accumulation depth, one rescale per iteration, and __expf of an argument of size up to R three
    # times (the term, the running rescale, the block rescale), each 2 R + 2 ulps (the argument's rounding is R u32); then
    # logf and the add of the maximum
    E_lse = lse.abs() + mx.abs() + ce_depth(dtype, V) + 2.0 * ce_iters(dtype, V) + 3.0 * (2.0 * R + 2.0)
    live = live_rows(labels, V)
    lab = torch.where(live, labels, torch.zeros_like(labels))
    row = torch.where(live, lse - x.gather(1, lab[:, None])[:, 0], torch.zeros_like(lse))
    return lse, E_lse, row, torch.where(live, E_lse + row.abs(), torch.zeros_like(lse))


def ce_reduce_reference(loss_row, E_row, labels):
    """-> (loss, E_loss [U32], count): the sum of the rows (ceil(T / 256) adds per thread + 9) over max(count, 1)."""
    T = loss_row.numel()
    count = int(counted_rows(labels).sum())
    den = max(count, 1)
    loss = loss_row.double().sum() / den
    depth = -(-T // 256) + 9 + 2
    return loss, (E_row.sum() + depth * loss_row.double().abs().sum()) / den + loss.abs(), count


def ce_bwd_reference(logits, labels, lse, count, gscale=None, ld=None):
    """lse: the stored fp32 values the kernel reads.  -> (dlogits [T, ld], E): zeros in [V, ld) and in rows that are not live."""
    dtype, (T, V) = logits.dtype, logits.shape
    ld = V if ld is None else ld
    x = logits.double()
    live = live_rows(labels, V)
    arg = x - lse.double()[:, None]
    p = torch.exp(arg)
    onehot = torch.zeros_like(p)
    onehot.scatter_(1, torch.where(live, labels, torch.zeros_like(labels))[:, None], 1.0)
    scale = (1.0 if gscale is None else float(gscale)) / max(float(count), 1.0)
    r = (p - onehot) * scale
    a = torch.where(torch.isfinite(arg), arg.abs(), torch.zeros_like(arg))
    e = r.abs() + _uscale(dtype) * (p * abs(scale) * (2.0 * a + 4.0) + 2.0 * r.abs())
    ref = torch.zeros(T, ld, dtype=torch.float64, device=x.device)
    E = torch.zeros_like(ref)
    ref[:, :V] = torch.where(live[:, None], r, torch.zeros_like(r))
    E[:, :V] = torch.where(live[:, None], e, torch.zeros_like(e))
    return ref, E


def check_ce(dtype, logits, labels, lse, lc, dlogits, gscale, loss_row=None, tag="ce"):
    """Every cross-entropy output against fp64: logits [T, V] (valid columns), lse [T], lc = (loss, count), dlogits [T, ld] (the
    whole storage rows: [V, ld) must be zero), loss_row [T] where the caller kept it."""
    V = logits.shape[1]
    lse64, El, row64, Er = ce_fwd_reference(logits, labels)
    bound(tag + " lse", "ce.lse", dtype, lse, lse64, El, u=U32)
    if loss_row is not None:
        bound(tag + " loss_row", "ce.loss_row", dtype, loss_row, row64, Er, u=U32)
        assert not bool(loss_row[~live_rows(labels, V)].any()), tag + ": an ignored row has a loss"
    loss64, Eloss, count = ce_reduce_reference(row64, Er, labels)
    assert float(lc[1]) == float(count), (tag, float(lc[1]), count)
    bound(tag + " loss", "ce.loss", dtype, lc[:1], loss64.reshape(1), Eloss.reshape(1), u=U32)
    live = live_rows(labels, V)
    assert not bool(dlogits[~live].any()), tag + ": an ignored row has a gradient"
    assert not bool(dlogits[:, V:].any()), tag + ": dlogits[:, V:ld] != 0"
    ref, E = ce_bwd_reference(logits, labels, lse, count, gscale, dlogits.shape[1])
    bound(tag + " dlogits", "ce.dlogits", dtype, dlogits, ref, E)


# ---- arg-max ---------------------------------------------------------------------------------------------------------------------
def argmax_chain(logits, temperature):
    """The documented chain: s = T(x / temp) (fp32 division, one rounding to T), p = T(softmax(s)), first index of max p.
    -> (index [rows], robust [rows]): robust = the elements that tie at the maximum of p are exactly those that tie at the maximum
    of s, so the index does not depend on the last bit of an exp or on the order of the softmax sum."""
    T = logits.dtype
    s = (logits.float() / torch.tensor(temperature, dtype=torch.float32, device=logits.device)).to(T).float()
    p = torch.softmax(s.double(), -1).float().to(T).float()
    pm, sm = p.max(-1, keepdim=True).values, s.max(-1, keepdim=True).values
    return (p == pm).int().argmax(-1), ((p == pm) == (s == sm)).all(-1)


def argmax_row(V, dtype, device, seed, ties, fill=None, neg_inf=()):
    """One row: normal values clamped to |x| <= 4, or the constant `fill`; the maximum 6.0 (well clear of the rest) at every index
    of `ties`; -inf at `neg_inf`."""
    if fill is None:
        x = torch.randn(V, generator=_gen(device, seed), device=device).clamp_(-4.0, 4.0)
    else:
        x = torch.full((V,), float(fill), device=device)
    for i in neg_inf:
        x[i] = float("-inf")
    for i in ties:
        x[i] = 6.0
    return x.to(dtype)


def argmax_tie_rows(V, dtype):
    """(name, ties, fill, neg_inf) of the constructed rows that exist at this V."""
    vn = VN[dtype]
    Vv = V // vn * vn
    pairs = [("ends", (0, V - 1)), ("vector", (7, 8)), ("stride", (8191, 8192)), ("chunk", (4095, 4096)), ("tail", (Vv - 1, Vv)),
             ("last", (V - 1,)), ("last_pair", (V - 2, V - 1))]
    rows = [(n, t, None, ()) for n, t in pairs if all(0 <= i < V for i in t)]
    rows.append(("all_equal", (), 1.5, ()))
    rows.append(("neg_inf", (V // 2, V - 1), None, tuple(range(0, min(V // 2, 40))) + (V - 2,)))
    return rows


# ---- outputs in caller-made views -----------------------------------------------------------------------------------------------
def guarded(shape, dtype, ld=None, extra_rows=0, device="cuda"):
    """an output [R, W] with row stride ld (default W) and `extra_rows` spare rows in a NaN-sentinel storage; 1-D for a 1-D shape.
    -> (view, Guarded)."""
    if len(shape) == 1:
        g = Guarded(shape[0], dtype, device)
        return g.view(shape, (1,)), g
    R, W = shape
    ld = W if ld is None else ld
    g = Guarded((R + extra_rows) * ld, dtype, device)
    return g.view((R, W), (ld, 1)), g


# ---- MoE expert fusion (mm_expert_fuse) -------------------------------------------------------------------------------------------
# expert_fuse_kernel: w_j = gate[n, idx[j]] (mode 1: the J-way softmax of those, expf(w - max) / sum, fp32), then
#   mode 0  out[n]    = T(sum_j w_j X[idx[j], n])   one fma per expert in fp32, ONE rounding
#   mode 1  out[n, j] = T(w'_j X[idx[j], n])         one product, ONE rounding
#   backward = 1: dX[idx[j], n] = T(w_j dout[n]) (mode 0) / T(w'_j dout[n, j]) (mode 1); the unlisted slices are not written.
# Error scale, kappa = U32 / u:  mode 0: E = |ref| + kappa (J + 2) sum_j |w_j x_j| (J adds, the product, the store);
#                                mode 1: E = |ref| (1 + kappa (J + 8))  (expf, the J-term sum and the divide of the softmax).
FUSE_MAXJ = 16                       # MOE_MAXJ


def _fuse_weights(gate, idx, mode):
    w = gate.double()[:, list(idx)]                                        # [n, J]
    return torch.softmax(w, -1) if mode == 1 else w


def expert_fuse_reference(X, gate, idx, mode):
    """X [E, n, L] (stored), gate [n, E] fp32, idx the listed experts.  -> (ref, E): [n, L] (mode 0) / [n, J, L] (mode 1), fp64."""
    J, kappa = len(idx), _uscale(X.dtype)
    w = _fuse_weights(gate, idx, mode)
    terms = w[:, :, None] * X.double()[list(idx)].permute(1, 0, 2)          # [n, J, L]
    if mode == 0:
        ref = terms.sum(1)
        return ref, ref.abs() + kappa * (J + 2) * terms.abs().sum(1)
    return terms, terms.abs() * (1.0 + kappa * (J + 8))


def expert_fuse_bwd_reference(dout, gate, idx, mode, E_experts):
    """dout [n, L] (mode 0) / [n, J, L] (mode 1).  -> (dX, E) [E_experts, n, L] in fp64; the slices of experts that are not listed
    are zero here with E = 0 -- the kernel does not write them, so a caller compares the listed slices only."""
    J, kappa = len(idx), _uscale(dout.dtype)
    w = _fuse_weights(gate, idx, mode)
    d = dout.double()
    n, L = d.shape[0], d.shape[-1]
    ref = torch.zeros(E_experts, n, L, dtype=torch.float64, device=d.device)
    for j, e in enumerate(idx):
        ref[e] = w[:, j, None] * (d if mode == 0 else d[:, j])
    return ref, ref.abs() * (1.0 + kappa * ((J + 2) if mode == 0 else (J + 8)))


def expert_fuse_problem(E_experts, idx, n, L, dtype, mode, device, seed, exact=False):
    """X [E, n, L], gate [n, E] fp32 (softmax weights of random logits), dout in the mode's output shape.  With E = 3 and mode 1
    the first gate row is [90, 50, 10]: without the max subtraction expf overflows, with it the weights are 1, e^-40, e^-80.
    exact: X and dout small integers and every gate entry 0.25 -- mode 0 is then exact in fp32, and so is mode 1 when J is a
    power of two (the softmax is exactly 1 / J): the output is ONE rounding of the fp64 result."""
    g = _gen(device, seed)
    J = len(idx)
    oshape = (n, L) if mode == 0 else (n, J, L)
    if exact:
        X = torch.randint(-4, 5, (E_experts, n, L), generator=g, device=device).to(dtype)
        dout = torch.randint(-4, 5, oshape, generator=g, device=device).to(dtype)
        gate = torch.full((n, E_experts), 0.25, device=device)
    else:
        # |x| >= 2^-6: the smallest weight of the range row, e^-80 = 1.8e-35, times x then stays a NORMAL number (>= 2.8e-37) in
        # bf16 and fp32 alike -- the rule's u is a relative roundoff and does not describe a subnormal result
        away = lambda t: torch.where(t < 0, -1.0, 1.0) * t.abs().clamp_min(2.0 ** -6)
        X = away(torch.randn(E_experts, n, L, generator=g, device=device)).to(dtype)
        dout = away(torch.randn(*oshape, generator=g, device=device)).to(dtype)
        gate = torch.softmax(2.0 * torch.randn(n, E_experts, generator=g, device=device), -1)
        if E_experts == 3 and mode == 1:
            gate[0] = torch.tensor([90.0, 50.0, 10.0], device=device)
    return X, gate, dout


def fuse_listed(t, idx):
    """the listed experts' slices of a [E, n, L] tensor, in idx order: [J, n, L]"""
    return t[list(idx)]


# ---- grouped LayerNorm / reduce (mm_layernorm_*_batched, mm_reduce_partials2_batched) ---------------------------------------------
# One expert-major buffer [groups * R, H]; expert g's rows are checked against the fp64 LayerNorm of ITS slice with ITS w / b under
# the stand-alone constants C["layernorm.*"] (the arithmetic is the stand-alone kernel's), recorded under grouped.layernorm.*.
# Every expert has its own seed and its own w / b ramp (sign and slope change with g), so another expert's weights are far off.
# Measured over tests/test_grouped_contract_gpu.py (bf16, f32), against the c of C["layernorm.*"]: mean 0.074, 0.204; rstd 0.233,
# 0.219; y 0.996, 0.240; dx 0.996, 0.387; dw 0.995, 0.139; db 0.995, 0.105.
def grouped_norm_problem(groups, R, H, dtype, device, seed):
    """-> dict: x, dy, dres [groups * R, H] expert-major, ws / bs = per-expert [H] (all in the storage dtype)"""
    ps = [norm_problem(R, H, dtype, device, seed + 7919 * g, layer=True) for g in range(groups)]
    slope = lambda g: (1.0 + 0.25 * g) * (-1.0 if g % 2 else 1.0)
    cat = lambda k: torch.cat([p[k] for p in ps]) if groups * R else ps[0][k][:0]
    return {"x": cat("x"), "dy": cat("dy"), "dres": cat("dres"),
            "ws": [(p["w"].float() * slope(g)).to(dtype) for g, p in enumerate(ps)],
            "bs": [(p["b"].float() + 0.5 * g * slope(g)).to(dtype) for g, p in enumerate(ps)]}


GROUPED_PREFIX = ["grouped"]         # tests/test_grouped_check_cpu.py records its emulation under "grouped_emulation" instead


def _gbound(name, kernel, dtype, got, ref, E, u=None):
    return check_bound(name, got, ref.to(got.device), E.to(got.device), c_of(kernel, dtype), U[dtype] if u is None else u,
                       key=f"{GROUPED_PREFIX[0]}.{kernel}.{NAME[dtype]}", log=RATIOS)


def check_grouped_layernorm_fwd(tag, x, ws, bs, eps, R, y, mean, rstd):
    """y, mean, rstd [groups * R (, H)] of mm_layernorm_fwd_batched, expert by expert"""
    dtype = x.dtype
    for g in range(len(ws)):
        sl = slice(g * R, (g + 1) * R)
        y64, Ey, m64, Em, r64, Er = layernorm_fwd_reference(x[sl], ws[g], bs[g], eps)
        _gbound(f"{tag} mean, expert {g}", "layernorm.mean", dtype, mean[sl], m64, Em, u=U32)
        _gbound(f"{tag} rstd, expert {g}", "layernorm.rstd", dtype, rstd[sl], r64, Er, u=U32)
        _gbound(f"{tag} y, expert {g}", "layernorm.y", dtype, y[sl], y64, Ey)


def check_grouped_layernorm_bwd(tag, dy, x, ws, mean, rstd, dres, R, dx, dws, dbs):
    """dx [groups * R, H] and the reduced per-expert dws[g] / dbs[g] [H] of mm_layernorm_bwd_batched + mm_reduce_partials2_batched
    (overwrite), from the STORED mean / rstd"""
    dtype = x.dtype
    for g in range(len(ws)):
        sl = slice(g * R, (g + 1) * R)
        dx64, Edx, dw64, Edw, db64, Edb = layernorm_bwd_reference(dy[sl], x[sl], ws[g], mean[sl], rstd[sl], dres[sl] if dres is not None else None)
        _gbound(f"{tag} dx, expert {g}", "layernorm.dx", dtype, dx[sl], dx64, Edx)
        _gbound(f"{tag} dw, expert {g}", "layernorm.dw", dtype, dws[g], dw64, Edw)
        _gbound(f"{tag} db, expert {g}", "layernorm.db", dtype, dbs[g], db64, Edb)


def grouped_partials_problem(groups, nblk, H, device, seed, extra_rows=2):
    """the exact family of partials_problem per expert: partials [groups * nblk + extra_rows, H] f32 expert-major (expert g + 1's
    blocks follow expert g's; NaN in the rows past the last expert's) -> (p, [before_g], [q_g])"""
    ps = [partials_problem(nblk, H, device, seed + 7919 * g) for g in range(groups)]
    p = torch.full((groups * nblk + extra_rows, H), float("nan"), dtype=F32, device=device)
    for g, (pg, _, _) in enumerate(ps):
        p[g * nblk:(g + 1) * nblk] = pg
    return p, [b for _, b, _ in ps], [q for _, _, q in ps]


def check_grouped_partials(tag, p, befores, qs, nblk, accumulate, outs, dtype):
    """outs[g] == the ONE rounding of the fp64 sum of expert g's nblk blocks (+ what it held), bitwise"""
    for g, out in enumerate(outs):
        want = rne(partials_reference(p[g * nblk:(g + 1) * nblk], qs[g], befores[g] if accumulate else None), dtype)
        check_exact(f"{tag} expert {g}", out, want.to(out.device))
