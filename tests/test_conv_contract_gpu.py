"""The NHWC convolution kernels of the MoE gate (csrc/mm_conv.hip) against their contract (include/mm_hip.h), on the GPU.

mm_conv2d_nhwc_fwd: six cases that cross every boundary of the kernel (the 7x7 stem on 3 real + 5 zero channels, both 3x3 strides,
the 1x1 expand with residual + ReLU, the strided 1x1 downsample without ReLU, 8 cout tiles over a K of 4608), each on n = 2 odd,
non-square images (ragged pixel tiles, both borders), outputs in NaN-sentinel guarded storages, in two families: exact (bit for bit)
and random (per-element fp64 bound, tests/conv_check.py).  mm_nchw_to_nhwc and mm_maxpool2d_nhwc: exact equality.  mm_gate_head: the
per-element fp64 bound and exact top-k indices."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_check as CC
from tests.kernel_check import Guarded, U

pytestmark = pytest.mark.gpu

# name: (H, W, Cin, Cout, R, stride, pad, residual, relu, real_cin)
CASES = {
    "stem": (37, 29, 8, 64, 7, 2, 3, False, False, 3),
    "3x3": (9, 7, 64, 64, 3, 1, 1, False, False, None),
    "3x3-strided": (9, 7, 128, 128, 3, 2, 1, False, False, None),      # -> 5x4: M = 40, under one tile
    "1x1-expand": (9, 7, 64, 256, 1, 1, 0, True, True, None),
    "downsample": (9, 7, 256, 512, 1, 2, 0, False, False, None),
    "multi-tile": (3, 2, 512, 512, 3, 1, 1, False, False, None),
}
DTYPES = [torch.bfloat16, torch.float32]


def _case(name, dtype, family):
    H, W, Cin, Cout, R, stride, pad, residual, relu, real_cin = CASES[name]
    return CC.make_case(2, H, W, Cin, Cout, R, stride, pad, residual, relu, dtype, family, seed=sorted(CASES).index(name),
                        real_cin=real_cin, device="cuda")


def _args(case):
    return (case["x"], case["w"], case["scale"], case["shift"], case["residual"], case["relu"], case["stride"], case["pad"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_conv_exact_family(name, dtype):
    case = _case(name, dtype, "exact")
    ref = CC.exact_reference(*_args(case))
    y, guard = CC.run_conv(case)
    torch.cuda.synchronize()
    guard.verify(f"{name} y")
    CC.check_exact(f"{name} {dtype}", y, ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_conv_random_family(name, dtype):
    case = _case(name, dtype, "random")
    ref, E, _ = CC.reference(*_args(case))
    y, guard = CC.run_conv(case)
    torch.cuda.synchronize()
    guard.verify(f"{name} y")
    path = CC.path_of(dtype)
    CC.check(f"{name} {path}", y, ref, E, CC.C[path]["conv"], U[dtype], path, "conv")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_nchw_to_nhwc_exact(dtype):
    from multimeditron_amd import kernels as K
    px = torch.randn(2, 3, 37, 29, generator=torch.Generator().manual_seed(1)).cuda()
    out = K.nchw_to_nhwc(px, 8, dtype)
    assert out.shape == (2, 37, 29, 8)
    assert torch.equal(out[..., :3], px.permute(0, 2, 3, 1).to(dtype))
    assert bool((out[..., 3:].view(torch.int16 if dtype == torch.bfloat16 else torch.int32) == 0).all())      # +0, bit for bit


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_maxpool_exact(dtype):
    from multimeditron_amd import kernels as K
    x = torch.randn(2, 9, 7, 64, generator=torch.Generator().manual_seed(2)).to(dtype).cuda()
    x = x - 3.0                                  # mostly negative: a padding tap counted as 0 would win the maximum
    gd = Guarded(2 * 5 * 4 * 64, dtype, x.device)
    y = K.maxpool2d_nhwc(x, out=gd.view((2, 5, 4, 64), (5 * 4 * 64, 4 * 64, 64, 1)))
    torch.cuda.synchronize()
    gd.verify("maxpool y")
    want = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).to(dtype)
    assert torch.equal(y, want)


@pytest.mark.parametrize("top_k", [1, 5])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_gate_head(dtype, top_k):
    from multimeditron_amd import kernels as K
    g = torch.Generator().manual_seed(3)
    n, HW, C, E = 3, 6, 2048, 5
    x = torch.relu(torch.randn(n, HW, C, generator=g)).to(dtype).cuda()
    fc_w = (torch.randn(E, C, generator=g) * C ** -0.5).to(dtype).cuda()
    fc_b = (4.0 * torch.arange(E).float()).flip(0).roll(2).to(dtype).cuda()          # a non-monotone order: 4, 0, 16, 12, 8
    ref = CC.head_reference(x, fc_w, fc_b, top_k)
    logits, topk, weights = K.gate_head(x, fc_w, fc_b, top_k)
    torch.cuda.synchronize()
    path = CC.path_of(dtype)
    CC.check(f"head logits {path}", logits, ref["logits"], ref["E_logits"], CC.C[path]["logits"], U[dtype], path, "logits")
    CC.check(f"head weights {path}", weights, ref["weights"], ref["E_weights"], CC.C[path]["weights"], U[dtype], path, "weights")
    assert topk.dtype == torch.int64 and torch.equal(topk, ref["topk"])
