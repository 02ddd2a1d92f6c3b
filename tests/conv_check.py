"""Checker for the NHWC convolution kernels (csrc/mm_conv.hip; the contract is in include/mm_hip.h): an fp64 reference with a
per-element error scale, an exact family, and guarded launches.  Works on any device: tests/test_conv_check_cpu.py feeds it
corrupted references on the CPU to show which kernel mistakes it rejects.

y[n, Ho, Wo, Cout] = act(conv(x[n, H, W, Cin], w[Cout, R, S, Cin]) * scale + shift (+ residual)), computed in float64 on the SAME
storage-rounded x, w, residual and fp32 scale / shift the kernel reads.

Random family: the rule of tests/kernel_check.py (`check`, c in `C` below) with
    E = |ref| + K (u32 / u) |scale| (|x| (*) |w|),      K = R S Cin,   (*) = the same convolution on absolute values:
the one rounding at the store (|ref|) plus a worst-case bound on the fp32 accumulation of K exact products carried through the
scale.

Exact family: integer x and w with |.| <= 4, a power-of-two scale per channel, integer shift and residual, so that every fp32
partial sum in any order is exact (`exact_reference` asserts it: the sum of |terms| stays below 2^24 and the fp64 result is an fp32
number).  The bf16 result must then equal bf16(fp64) bit for bit and the fp32 result the fp64 value."""
import torch
import torch.nn.functional as F

from tests.kernel_check import U, U32, Guarded, RatioLog, check_bits, check_bound

# c per storage type and quantity (conv: the six contract cases; head: mm_gate_head's logits and weights); measured worst
# err / (u E) on the MI355X beside each
C = {
    "bf16": {"conv": 2.0, "logits": 2.0, "weights": 2.0},                    # measured 0.979, 0.835, 0.527
    "f32": {"conv": 0.125, "logits": 2.0 ** -11, "weights": 2.0 ** -11},     # measured 0.0318, 1.68e-4, 1.56e-4 (K and C + HW are worst-case factors)
}
RATIOS = RatioLog("MM_CONV_RATIO_LOG")


def path_of(dtype):
    return "bf16" if dtype == torch.bfloat16 else "f32"


def out_size(size, R, stride, pad):
    return (size + 2 * pad - R) // stride + 1


def reference(x, w, scale, shift, residual, relu, stride, pad):
    """fp64 on x's device.  x [n, H, W, Cin], w [Cout, R, S, Cin], scale / shift [Cout], residual [n, Ho, Wo, Cout] or None ->
    (ref, E, absacc), all [n, Ho, Wo, Cout] float64; absacc = |x| (*) |w|."""
    xd, wd = x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2)
    K = w.shape[1] * w.shape[2] * w.shape[3]
    acc = F.conv2d(xd, wd, None, stride, pad).permute(0, 2, 3, 1)
    absacc = F.conv2d(xd.abs(), wd.abs(), None, stride, pad).permute(0, 2, 3, 1)
    ref = acc * scale.double() + shift.double()
    if residual is not None:
        ref = ref + residual.double()
    if relu:
        ref = F.relu(ref)
    kappa = U32 / U[x.dtype]
    E = ref.abs() + K * kappa * scale.double().abs() * absacc
    return ref.contiguous(), E.contiguous(), absacc.contiguous()


def exact_reference(x, w, scale, shift, residual, relu, stride, pad):
    """The exact family's reference: asserts that every partial sum of the kernel is exact in fp32, whatever the order."""
    ref, _E, absacc = reference(x, w, scale, shift, residual, relu, stride, pad)
    for t in (x, w, shift) + ((residual,) if residual is not None else ()):
        assert bool((t.double() == t.double().round()).all()), "exact family: integer operands"
    m, e = torch.frexp(scale.double().abs())
    assert bool((m == 0.5).all()), "exact family: power-of-two scales"
    total = absacc * scale.double().abs() + shift.double().abs()
    if residual is not None:
        total = total + residual.double().abs()
    assert float(absacc.max()) < 2.0 ** 24 and float(total.max()) < 2.0 ** 24, "exact family: partial sums must stay exact in fp32"
    assert bool((ref.float().double() == ref).all())
    return ref


def check(name, got, ref, E, c, u, path=None, quantity="conv"):
    """The rule; the worst err / (u E) is recorded in RATIOS[(path, quantity)]."""
    return check_bound(name, got, ref, E, c, u, key=path and (path, quantity), log=RATIOS)


def check_exact(name, got, ref):
    """The exact family: got == T(ref) (ref is an fp32 number, so the rounding to T is a single one), a zero of either sign."""
    check_bits(name, got, ref.to(torch.float32).to(got.dtype), zero_sign=False)


# ---- operands -----------------------------------------------------------------------------------------------------------
def make_case(n, H, W, Cin, Cout, R, stride, pad, residual, relu, dtype, family, seed=0, real_cin=None, device="cpu"):
    """Operands of one contract case.  family 'exact' | 'random'.  real_cin: channels real_cin .. Cin-1 of x and w are zero (the
    stem's 3 -> 8 padding)."""
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = out_size(H, R, stride, pad), out_size(W, R, stride, pad)
    if family == "exact":
        x = torch.randint(-4, 5, (n, H, W, Cin), generator=g).float()
        w = torch.randint(-4, 5, (Cout, R, R, Cin), generator=g).float()
        scale = 2.0 ** torch.randint(-3, 2, (Cout,), generator=g).float() * (1 - 2 * torch.randint(0, 2, (Cout,), generator=g)).float()
        shift = torch.randint(-8, 9, (Cout,), generator=g).float()
        res = torch.randint(-8, 9, (n, Ho, Wo, Cout), generator=g).float() if residual else None
    else:
        x = torch.randn(n, H, W, Cin, generator=g)
        w = torch.randn(Cout, R, R, Cin, generator=g) * (R * R * Cin) ** -0.5
        scale = (torch.rand(Cout, generator=g) + 0.5) * (1 - 2 * torch.randint(0, 2, (Cout,), generator=g)).float()
        shift = torch.randn(Cout, generator=g) * 0.5
        res = torch.randn(n, Ho, Wo, Cout, generator=g) if residual else None
    if real_cin is not None:
        x[..., real_cin:] = 0
        w[..., real_cin:] = 0
    x, w = x.to(dtype).to(device), w.to(dtype).to(device)
    res = res.to(dtype).to(device) if res is not None else None
    return dict(x=x, w=w, scale=scale.to(device), shift=shift.to(device), residual=res, relu=relu, stride=stride, pad=pad)


# ---- guarded launch -------------------------------------------------------------------------------------------------------
def run_conv(case):
    """mm_conv2d_nhwc_fwd with y inside a guarded storage; returns (y, guard)."""
    from multimeditron_amd import kernels as K
    x, w = case["x"], case["w"]
    n, H, W, _ = x.shape
    Cout, R = w.shape[0], w.shape[1]
    Ho, Wo = out_size(H, R, case["stride"], case["pad"]), out_size(W, R, case["stride"], case["pad"])
    gd = Guarded(n * Ho * Wo * Cout, x.dtype, x.device)
    y = gd.view((n, Ho, Wo, Cout), (Ho * Wo * Cout, Wo * Cout, Cout, 1))
    K.conv2d_nhwc(x, w, case["scale"], case["shift"], case["stride"], case["pad"], residual=case["residual"], relu=case["relu"], out=y)
    return y, gd


# ---- mm_gate_head ---------------------------------------------------------------------------------------------------------
def head_reference(x, fc_w, fc_b, top_k):
    """fp64 reference of mm_gate_head on x [n, HW, C]: -> dict(logits, E_logits, weights, E_weights, topk).
    E_logits = |l| + (C + HW) (u32 / u) (mean|x| . |w| + |b|): the rounding of the logit plus the fp32 mean and dot product;
    E_weights = |p| + p_e (E_l[e] + sum_j p_j E_l[j]): the rounding of the weight plus the logits' error carried through the softmax
    (d p_e = p_e (d l_e - sum_j p_j d l_j))."""
    n, HW, C = x.shape
    xd, wd, bd = x.double(), fc_w.double(), fc_b.double()
    kappa = U32 / U[x.dtype]
    logits = xd.mean(1) @ wd.t() + bd
    E_l = logits.abs() + (C + HW) * kappa * (xd.abs().mean(1) @ wd.abs().t() + bd.abs())
    p = torch.softmax(logits, dim=-1)
    E_p = p + p * (E_l + (p * E_l).sum(-1, keepdim=True))
    return dict(logits=logits, E_logits=E_l, weights=p, E_weights=E_p, topk=logits.topk(top_k, dim=-1).indices)
