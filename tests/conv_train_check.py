"""Checker for the kernels that train the MoE gate (csrc/mm_conv_bwd.hip, mm_expert_fuse_gate_bwd; contracts in include/mm_hip.h):
fp64 references with per-element error scales, exact families, fp32 restatements and guarded launches.  Works on any device:
tests/test_conv_train_check_cpu.py feeds it restatements with one planted mistake each.

Every check is LOCAL: one launch, fed the storage-rounded operands that launch read (for the BatchNorm backward that includes the
fp32 mean / invstd the forward wrote), held to the rule of tests/kernel_check.py with c = 2 for both storage types.  The error
scales E are sums of absolute values of fp64 terms, one per rounding point, in units of the OUTPUT's unit roundoff u; an fp32 term
enters a bf16 output's E scaled by kappa = u32 / u.  None is fitted to kernel output.

Column sums over M (BatchNorm): the contract bounds the number of additions an element passes through by D(M) = 21 + ceil(M / 512),
so a sum's fp32 error is at most D u32 sum|terms|.  The cancellation of the BatchNorm backward (two means subtracted from a
nearly uniform gradient) lands in E through |sum g| / M and |xhat| |sum g xhat| / M.
Convolution gradients: K exact products accumulated in fp32 in any order: K u32 (|a| (*) |b|), plus the output rounding.
E = 0 means equality: pixels no output reads (stride-2 1x1 data gradient), the stem's padded channels, unlisted experts, max-pool
positions that win no window, and dres (the bits of dy or zero)."""
import math

import torch
import torch.nn.functional as F

from tests.kernel_check import U, U32, Guarded, RatioLog, check_bits, check_bound

# c = 2 for both storage types (E is a worst case, a correct kernel stays near or under 1); the worst err / (u E) measured on the
# MI355X over tests/test_conv_train_contract_gpu.py beside each quantity
C = 2.0
MEASURED = {
    "bf16": {"bn.mean": 0.035, "bn.invstd": 0.22, "bn.y": 0.995, "bn.running_mean": 0.995, "bn.running_var": 0.983, "bn.dz": 0.995,
             "bn.dgamma": 0.987, "bn.dbeta": 0.988, "bn.dres": 0.0, "dgrad": 0.989, "wgrad": 0.994, "pool.dx": 0.981, "dgate": 1.7e-3,
             "gate.bn.dz": 0.996, "gate.bn.dgamma": 0.984, "gate.bn.dbeta": 0.995, "gate.dgrad": 0.994, "gate.wgrad": 0.996,
             "gate.pool": 0.996},                        # bf16: the output rounding dominates, so a correct kernel sits just under 1
    "f32": {"bn.mean": 0.091, "bn.invstd": 0.22, "bn.y": 0.117, "bn.running_mean": 0.465, "bn.running_var": 0.537, "bn.dz": 0.305,
            "bn.dgamma": 0.083, "bn.dbeta": 0.064, "bn.dres": 0.0, "dgrad": 0.024, "wgrad": 0.136, "pool.dx": 0.469, "dgate": 1.4e-3,
            "gate.bn.dz": 0.390, "gate.bn.dgamma": 0.118, "gate.bn.dbeta": 0.082, "gate.dgrad": 0.052, "gate.wgrad": 0.286,
            "gate.pool": 0.544},                         # dgate: L is a worst-case factor on a sum of L terms
}
RATIOS = RatioLog("MM_CONV_TRAIN_RATIO_LOG")
BN_EPS = 1e-5
BN_ROWS = 512
WGRAD_ROWS = 1024


def path_of(dtype):
    return "bf16" if dtype == torch.bfloat16 else "f32"


def check(name, got, ref, E, quantity, dtype=None, u=None):
    """The rule with c = 2; dtype = the OUTPUT's dtype (u from it).  The worst ratio is recorded under (storage path, quantity)."""
    dtype = dtype or got.dtype
    return check_bound(name, got, ref, E, C, u or U[dtype], key=(path_of(dtype), quantity), log=RATIOS)


def check_exact(name, got, ref):
    check_bits(name, got, ref.to(torch.float32).to(got.dtype), zero_sign=False)


def bn_depth(M):
    return 21 + math.ceil(M / BN_ROWS)


# ---- BatchNorm, training forward -------------------------------------------------------------------------------------------------
def bn_fwd_reference(z, gamma, beta, residual, relu, eps=BN_EPS):
    """fp64 from the stored z [M, C] (T), gamma / beta [C] (T), residual [M, C] or None.  -> dict of (ref, E) pairs:
    mean, invstd (fp32 outputs: E in u32 units), y (T units), plus var / unbiased var for the running statistics."""
    M = z.shape[0]
    zd, g, b = z.double(), gamma.double(), beta.double()
    kappa = U32 / U[z.dtype]
    D = bn_depth(M)
    Dm = D + 4 * math.ceil(M / BN_ROWS)                 # the merge of the workgroups' means adds a few operations per workgroup
    mean = zd.mean(0)
    dev = zd - mean
    var = (dev * dev).mean(0)
    absmean = zd.abs().mean(0)
    E_mean = Dm * absmean
    # sum (z - m')^2 / M = var + (m' - m)^2 exactly, so the mean's error enters squared; each squared deviation carries 2 roundings
    E_var = 2 * (Dm + 2) * var + U32 * (Dm * absmean) ** 2
    invstd = (var + eps) ** -0.5
    E_invstd = invstd * (3 + 0.5 * E_var / (var + eps))
    xhat = dev * invstd
    pre = xhat * g + b
    if residual is not None:
        pre = pre + residual.double()
    y = F.relu(pre) if relu else pre
    E_y = pre.abs() + kappa * (g.abs() * invstd * (E_mean + 2 * dev.abs()) + g.abs() * dev.abs() * E_invstd + 2 * (xhat * g).abs()
                               + b.abs() + 2 * pre.abs() + (residual.double().abs() if residual is not None else 0))
    unb = var * M / (M - 1)
    return dict(mean=(mean, E_mean), var=(var, E_var), invstd=(invstd, E_invstd), y=(y, E_y), unbiased=(unb, E_var * M / (M - 1) + 2 * unb))


def bn_running_reference(running, batch, E_batch, momentum=0.1):
    """running' = T((1 - momentum) * float(running) + momentum * batch): (ref, E) in T units; E_batch in u32 units."""
    r = running.double()
    kappa = U32 / U[running.dtype]
    ref = (1 - momentum) * r + momentum * batch
    return ref, ref.abs() + kappa * (2 * (1 - momentum) * r.abs() + 2 * momentum * batch.abs() + momentum * E_batch)


def bn_fwd_emulate(z, gamma, beta, residual, relu, eps=BN_EPS, mistake=None):
    """The contract restated in fp32 torch arithmetic with its rounding points.  mistake 'naive-var': var = E[z^2] - mean^2."""
    z32 = z.float()
    mean = z32.mean(0)
    if mistake == "naive-var":
        var = (z32 * z32).mean(0) - mean * mean
    else:
        var = ((z32 - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    v = (z32 - mean) * invstd * gamma.float() + beta.float()
    if residual is not None:
        v = v + residual.float()
    if relu:
        v = F.relu(v)
    return v.to(z.dtype), mean, invstd, var


# ---- BatchNorm, backward ---------------------------------------------------------------------------------------------------------
def bn_bwd_reference(dy, y, z, mean, invstd, gamma, relu):
    """fp64 from the operands the launch read: dy, y, z (T), mean / invstd (the fp32 the forward wrote), gamma (T).
    -> dict of (ref, E): dz, dres, dgamma, dbeta, all in T units."""
    M = z.shape[0]
    kappa = U32 / U[z.dtype]
    D = bn_depth(M)
    g = dy.double() * (y.double() > 0) if relu else dy.double()
    gm, istd = gamma.double(), invstd.double()
    xhat = (z.double() - mean.double()) * istd
    S1, S2 = g.sum(0), (g * xhat).sum(0)
    E_S1, E_S2 = D * g.abs().sum(0), (D + 3) * (g * xhat).abs().sum(0)
    t1, t2, t3 = g.abs(), S1.abs() / M, (xhat * S2).abs() / M
    dz = gm * istd * (g - S1 / M - xhat * S2 / M)
    E_dz = dz.abs() + kappa * (gm * istd).abs() * (4 * (t1 + t2 + t3) + 3 * t3 + E_S1 / M + xhat.abs() * E_S2 / M)
    return dict(dz=(dz, E_dz), dres=(g, torch.zeros_like(g)), dbeta=(S1, S1.abs() + kappa * E_S1), dgamma=(S2, S2.abs() + kappa * E_S2))


def bn_bwd_emulate(dy, y, z, mean, invstd, gamma, relu, mistake=None):
    """fp32 restatement.  mistakes: 'no-xhat-term' (dz without xhat sum(g xhat) / M), 'mask-from-z' (ReLU mask z > 0 instead of
    y > 0), 'early-rounding' (gamma invstd g rounded to T before the means are subtracted)."""
    T = z.dtype
    M = z.shape[0]
    if relu:
        mask = (z.float() > 0) if mistake == "mask-from-z" else (y.float() > 0)
        g = dy.float() * mask
    else:
        g = dy.float()
    xhat = (z.float() - mean) * invstd
    S1, S2 = g.sum(0), (g * xhat).sum(0)
    k = gamma.float() * invstd
    if mistake == "no-xhat-term":
        dz = k * (g - S1 / M)
    elif mistake == "early-rounding":
        dz = (k * g).to(T).float() - k * (S1 / M + xhat * S2 / M)
    else:
        dz = k * (g - S1 / M - xhat * (S2 / M))
    return dz.to(T), g.to(T), S2.to(T), S1.to(T)


def bn_case(M, C, dtype, residual, relu, seed=0, device="cpu"):
    """z [M, C] with channel 0 constant (variance 0) and channel 1 of mean 100, standard deviation 0.01; gamma, beta, residual,
    running statistics, dy."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(M, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g)
    z[:, 0] = 0.75
    z[:, 1] = 100.0 + 0.01 * torch.randn(M, generator=g)
    gamma = (0.5 + torch.rand(C, generator=g)) * (1 - 2 * torch.randint(0, 2, (C,), generator=g)).float()
    beta = 0.5 * torch.randn(C, generator=g)
    res = torch.randn(M, C, generator=g) if residual else None
    rm, rv = torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    dy = torch.randn(M, C, generator=g)
    to = lambda t: None if t is None else t.to(dtype).to(device)
    return dict(z=to(z), gamma=to(gamma), beta=to(beta), residual=to(res), relu=relu, running_mean=to(rm), running_var=to(rv),
                num_batches_tracked=torch.tensor(7, dtype=torch.int64, device=device), dy=to(dy))


# ---- convolution gradients ---------------------------------------------------------------------------------------------------------
def out_size(size, R, stride, pad):
    return (size + 2 * pad - R) // stride + 1


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def dgrad_reference(dz, w, H, W, stride, pad, addend=None):
    """dz [n, Ho, Wo, Cout], w [Cout, R, S, Cin] (T) -> (dx fp64 [n, H, W, Cin], E)."""
    n, Cout = dz.shape[0], dz.shape[3]
    R, Cin = w.shape[1], w.shape[3]
    size = (n, Cin, H, W)
    wd = w.double().permute(0, 3, 1, 2)
    ref = torch.nn.grad.conv2d_input(size, wd, _nchw(dz), stride=stride, padding=pad).permute(0, 2, 3, 1)
    absacc = torch.nn.grad.conv2d_input(size, wd.abs(), _nchw(dz).abs(), stride=stride, padding=pad).permute(0, 2, 3, 1)
    kappa = U32 / U[dz.dtype]
    E = kappa * R * R * Cout * absacc
    if addend is not None:
        ref = ref + addend.double()
        E = E + kappa * addend.double().abs()
    return ref.contiguous(), (ref.abs() + E).contiguous()


def wgrad_reference(dz, x, R, stride, pad):
    """dz [n, Ho, Wo, Cout], x [n, H, W, Cin] (T) -> (dw fp64 [Cout, R, R, Cin], E)."""
    Cout, Cin = dz.shape[3], x.shape[3]
    M = dz.shape[0] * dz.shape[1] * dz.shape[2]
    size = (Cout, Cin, R, R)
    ref = torch.nn.grad.conv2d_weight(_nchw(x), size, _nchw(dz), stride=stride, padding=pad).permute(0, 2, 3, 1)
    absacc = torch.nn.grad.conv2d_weight(_nchw(x).abs(), size, _nchw(dz).abs(), stride=stride, padding=pad).permute(0, 2, 3, 1)
    kappa = U32 / U[dz.dtype]
    return ref.contiguous(), (ref.abs() + kappa * M * absacc).contiguous()


def dgrad_emulate(dz, w, H, W, stride, pad, addend=None, mistake=None):
    """fp32 restatement.  mistakes: 'flipped-tap' (the filter mirrored), 'wrong-parity' (stride-2 taps landing one pixel off)."""
    n, Cin = dz.shape[0], w.shape[3]
    w32 = w.float().permute(0, 3, 1, 2)
    if mistake == "flipped-tap":
        w32 = w32.flip(2, 3)
    dx = torch.nn.grad.conv2d_input((n, Cin, H, W), w32, dz.float().permute(0, 3, 1, 2), stride=stride, padding=pad).permute(0, 2, 3, 1)
    if mistake == "wrong-parity":
        dx = torch.roll(dx, 1, dims=2)
    if addend is not None:
        dx = dx + addend.float()
    return dx.to(dz.dtype)


def wgrad_emulate(dz, x, R, stride, pad, mistake=None):
    """fp32 restatement: fp32 partials per run of 1024 output pixels, added in order, one rounding.  mistake 'split-dropped':
    the last run is left out."""
    n, Ho, Wo, Cout = dz.shape
    H, W, Cin = x.shape[1], x.shape[2], x.shape[3]
    # the runs cut the flattened pixel index, so scatter each run's rows of dz into a zero image and reuse the dense gradient
    flat = dz.float().reshape(-1, Cout)
    M = flat.shape[0]
    starts = list(range(0, M, WGRAD_ROWS))
    if mistake == "split-dropped":
        starts = starts[:-1]
    acc = torch.zeros(Cout, R, R, Cin)
    for s in starts:
        part = torch.zeros_like(flat)
        part[s:s + WGRAD_ROWS] = flat[s:s + WGRAD_ROWS]
        acc = acc + torch.nn.grad.conv2d_weight(x.float().permute(0, 3, 1, 2), (Cout, Cin, R, R),
                                                part.reshape(n, Ho, Wo, Cout).permute(0, 3, 1, 2), stride=stride,
                                                padding=pad).permute(0, 2, 3, 1)
    return acc.to(dz.dtype)


# name: (n, H, W, Cin, Cout, R, stride, pad, real_cin); the cases of the contract
CONV_CASES = {
    "1x1": (2, 8, 8, 64, 64, 1, 1, 0, None),
    "1x1-ragged": (3, 5, 7, 128, 256, 1, 1, 0, None),               # M = 105
    "3x3": (2, 9, 7, 64, 64, 3, 1, 1, None),
    "3x3-s2-odd": (2, 9, 8, 64, 128, 3, 2, 1, None),
    "3x3-s2-even": (2, 8, 8, 64, 128, 3, 2, 1, None),
    "1x1-s2": (2, 7, 7, 64, 256, 1, 2, 0, None),                    # -> 4x4: the odd input rows and columns are read by no output
    "stem": (2, 18, 18, 8, 64, 7, 2, 3, 3),                         # wgrad only
    "split-1x1": (4, 24, 24, 64, 64, 1, 1, 0, None),                # M = 2304: three runs of the weight gradient
    "split-3x3": (4, 24, 24, 64, 64, 3, 1, 1, None),
}


def conv_case(name, dtype, family, device="cpu", addend=False):
    """dz, x, w (packed [Cout, R, R, Cin]) and the optional addend of one case.  family 'exact': integers in [-2, 2], every partial
    sum exact in fp32 in any order (asserted by exact_sum_bound)."""
    n, H, W, Cin, Cout, R, stride, pad, real_cin = CONV_CASES[name]
    g = torch.Generator().manual_seed(sorted(CONV_CASES).index(name))
    Ho, Wo = out_size(H, R, stride, pad), out_size(W, R, stride, pad)
    if family == "exact":
        x = torch.randint(-2, 3, (n, H, W, Cin), generator=g).float()
        w = torch.randint(-2, 3, (Cout, R, R, Cin), generator=g).float()
        dz = torch.randint(-2, 3, (n, Ho, Wo, Cout), generator=g).float()
        add = torch.randint(-8, 9, (n, H, W, Cin), generator=g).float()
    else:
        x = torch.randn(n, H, W, Cin, generator=g)
        w = torch.randn(Cout, R, R, Cin, generator=g) * (R * R * Cin) ** -0.5
        dz = torch.randn(n, Ho, Wo, Cout, generator=g)
        add = torch.randn(n, H, W, Cin, generator=g)
    if real_cin is not None:
        x[..., real_cin:] = 0
        w[..., real_cin:] = 0
    to = lambda t: t.to(dtype).to(device)
    return dict(x=to(x), w=to(w), dz=to(dz), addend=to(add) if addend else None, H=H, W=W, R=R, stride=stride, pad=pad)


def exact_sum_bound(ref, E_terms):
    """exact family: the sum of |terms| stays below 2^24, so every fp32 partial sum is an integer it can hold."""
    assert float(E_terms.max()) < 2.0 ** 24 and bool((ref == ref.round()).all())


# ---- max-pool backward ---------------------------------------------------------------------------------------------------------------
def _pool_windows(x):
    """x [n, H, W, C] -> (onehot [n, C, 9, L] of the FIRST maximal real tap of each window, fold arguments)"""
    n, H, W, C = x.shape
    xd = F.pad(x.double().permute(0, 3, 1, 2), (1, 1, 1, 1), value=float("-inf"))
    Hp, Wp = xd.shape[2] - (xd.shape[2] - 3) % 2, xd.shape[3] - (xd.shape[3] - 3) % 2        # what the stride-2 windows cover
    cols = F.unfold(xd[:, :, :Hp, :Wp], 3, stride=2).reshape(n, C, 9, -1)
    real = F.unfold(F.pad(torch.ones(n, 1, H, W, dtype=torch.float64), (1, 1, 1, 1))[:, :, :Hp, :Wp], 3, stride=2).reshape(n, 1, 9, -1) > 0
    return cols, real.to(x.device), (Hp, Wp)


def maxpool_bwd_reference(x, dy, last=False):
    """fp64 gather of dy [n, Ho, Wo, C] onto the first (last=True: the LAST, the planted mistake) maximal element of each window,
    row-major window order; padding taps never win.  -> (dx [n, H, W, C], E)."""
    n, H, W, C = x.shape
    cols, real, (Hp, Wp) = _pool_windows(x)
    mx = cols.max(dim=2, keepdim=True).values
    ismax = (cols == mx) & real
    if last:
        ismax = ismax.flip(2)
    first = ismax & (ismax.cumsum(2) == 1)
    if last:
        first = first.flip(2)
    d = dy.double().permute(0, 3, 1, 2).reshape(n, C, 1, -1)

    def back(t):
        full = torch.zeros(n, C, H + 2, W + 2, dtype=torch.float64, device=x.device)
        full[:, :, :Hp, :Wp] = F.fold(t.reshape(n, C * 9, -1), (Hp, Wp), 3, stride=2)
        return full[:, :, 1:H + 1, 1:W + 1].permute(0, 2, 3, 1).contiguous()
    ref = back(first * d)
    wins = back(first.double().expand(n, C, 9, first.shape[3]))
    absd = back(first * d.abs())
    kappa = U32 / U[x.dtype]
    return ref, ref.abs() + kappa * (wins - 1).clamp(min=0) * absd


# ---- fusion: the gate's gradient ---------------------------------------------------------------------------------------------------
def gate_bwd_reference(X, dout, gate, idx, mode):
    """X [E, n, L] (T), dout [n, L] / [n, J, L] (T), gate [n, E] fp32 -> (dgate fp64 [n, E], E in u32 units)."""
    E_, n, L = X.shape
    J = len(idx)
    Xd, dd = X.double()[list(idx)], dout.double()                    # [J, n, L]
    dj = dd.unsqueeze(0) if mode == 0 else dd.permute(1, 0, 2)
    d = (dj * Xd).sum(-1).t()                                         # [n, J]
    Ed = L * (dj.abs() * Xd.abs()).sum(-1).t()
    if mode == 1:
        w = torch.softmax(gate.double()[:, list(idx)], dim=-1)
        dot = (w * d).sum(-1, keepdim=True)
        val = w * (d - dot)
        # the dot products' error through the linear map, plus the softmax (J + 8 roundings) and the few products here
        Ev = w * (Ed + (w * Ed).sum(-1, keepdim=True)) + (J + 12) * w * (d.abs() + (w * d.abs()).sum(-1, keepdim=True))
    else:
        val, Ev = d, d.abs() + Ed
    ref = torch.zeros(n, E_, dtype=torch.float64, device=X.device)
    Eo = torch.zeros_like(ref)
    for j, e in enumerate(idx):
        ref[:, e] += val[:, j]
        Eo[:, e] += Ev[:, j]
    return ref, Eo


def gate_bwd_emulate(X, dout, gate, idx, mode, mistake=None):
    """fp32 restatement.  mistake 'no-softmax-bwd': mode 1 returning the raw dot products."""
    E_, n, L = X.shape
    Xf = X.float()[list(idx)]
    dj = dout.float().unsqueeze(0) if mode == 0 else dout.float().permute(1, 0, 2)
    d = (dj * Xf).sum(-1).t()
    if mode == 1 and mistake != "no-softmax-bwd":
        w = torch.softmax(gate[:, list(idx)], dim=-1)
        d = w * (d - (w * d).sum(-1, keepdim=True))
    out = torch.zeros(n, E_)
    for j, e in enumerate(idx):
        out[:, e] += d[:, j]
    return out


# ---- guarded storages ------------------------------------------------------------------------------------------------------------------
def guarded(shape, dtype, device):
    """a contiguous tensor of `shape` inside a NaN-sentinel guarded storage -> (tensor, guard)"""
    numel = 1
    for s in shape:
        numel *= s
    gd = Guarded(numel, dtype, device)
    stride, acc = [], 1
    for s in reversed(shape):
        stride.append(acc)
        acc *= s
    return gd.view(tuple(shape), tuple(reversed(stride))), gd
