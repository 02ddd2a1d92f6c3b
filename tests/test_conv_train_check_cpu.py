"""Self-test of the gate-training checker (tests/conv_train_check.py) on the CPU, at the sizes the GPU contract tests use: the fp32
restatement of each contract passes with err / (u E) <= 1, and the same restatement with ONE planted mistake is rejected at c = 2:
the variance formed as E[z^2] - mean^2 (the mean-100 channel), a dropped xhat term, a ReLU mask taken from z instead of y, dz
rounded before the means are subtracted, a mirrored filter tap, a stride-2 tap of the wrong parity, a dropped M split, the last
maximal element of a pooling window instead of the first.

Two of the mistakes show in one storage type only, for a reason that lies in the number format and not in the checker: in bf16 a
channel of mean 100 and standard deviation 0.01 is stored as the constant 100 (the spacing there is 0.5), so E[z^2] - mean^2 is
exact; in fp32 storage an extra rounding "to T" is one more fp32 rounding among several."""
import pytest
import torch

from tests import conv_train_check as TC
from tests.kernel_check import U32

DTYPES = [torch.bfloat16, torch.float32]
IDS = ["bf16", "f32"]


def _bn_fwd(case, mistake=None):
    return TC.bn_fwd_emulate(case["z"], case["gamma"], case["beta"], case["residual"], case["relu"], mistake=mistake)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M", [2, 33, 4099])
@pytest.mark.parametrize("residual,relu", [(False, False), (True, True)])
def test_bn_forward_restatement_passes(M, dtype, residual, relu):
    case = TC.bn_case(M, 64, dtype, residual, relu, seed=M)
    ref = TC.bn_fwd_reference(case["z"], case["gamma"], case["beta"], case["residual"], relu)
    y, mean, invstd, _ = _bn_fwd(case)
    assert TC.check("mean", mean, *ref["mean"], "bn.mean", dtype, U32) <= 1.0
    assert TC.check("invstd", invstd, *ref["invstd"], "bn.invstd", dtype, U32) <= 1.0
    assert TC.check("y", y, *ref["y"], "bn.y", dtype) <= 1.0
    assert float(ref["var"][0][0]) == 0.0 and abs(float(ref["invstd"][0][0]) - TC.BN_EPS ** -0.5) < 1e-9      # the constant channel


@pytest.mark.parametrize("M", [33, 4099])
def test_bn_forward_rejects_the_naive_variance(M):
    case = TC.bn_case(M, 64, torch.float32, False, False, seed=M)
    ref = TC.bn_fwd_reference(case["z"], case["gamma"], case["beta"], None, False)
    y, mean, invstd, _ = _bn_fwd(case, "naive-var")
    with pytest.raises(AssertionError):
        TC.check("invstd", invstd, *ref["invstd"], "bn.invstd", torch.float32, U32)
    with pytest.raises(AssertionError):
        TC.check("y", y, *ref["y"], "bn.y", torch.float32)


def _bn_bwd_operands(M, dtype, residual, relu):
    case = TC.bn_case(M, 64, dtype, residual, relu, seed=M + 1)
    y, mean, invstd, _ = _bn_fwd(case)
    return case, y, mean, invstd


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M", [2, 33, 4099])
@pytest.mark.parametrize("relu", [False, True])
def test_bn_backward_restatement_passes(M, dtype, relu):
    case, y, mean, invstd = _bn_bwd_operands(M, dtype, relu, relu)
    ref = TC.bn_bwd_reference(case["dy"], y, case["z"], mean, invstd, case["gamma"], relu)
    dz, dres, dgamma, dbeta = TC.bn_bwd_emulate(case["dy"], y, case["z"], mean, invstd, case["gamma"], relu)
    for name, got in (("dz", dz), ("dres", dres), ("dgamma", dgamma), ("dbeta", dbeta)):
        assert TC.check(name, got, *ref[name], "bn." + name, dtype) <= 1.0


@pytest.mark.parametrize("M", [33, 4099])
@pytest.mark.parametrize("mistake,dtype", [("no-xhat-term", torch.bfloat16), ("no-xhat-term", torch.float32),
                                           ("mask-from-z", torch.bfloat16), ("mask-from-z", torch.float32),
                                           ("early-rounding", torch.bfloat16)])
def test_bn_backward_rejects_mistakes(mistake, dtype, M):
    case, y, mean, invstd = _bn_bwd_operands(M, dtype, True, True)      # a residual unit: y > 0 and z > 0 differ
    ref = TC.bn_bwd_reference(case["dy"], y, case["z"], mean, invstd, case["gamma"], True)
    dz, *_ = TC.bn_bwd_emulate(case["dy"], y, case["z"], mean, invstd, case["gamma"], True, mistake=mistake)
    with pytest.raises(AssertionError):
        TC.check("dz", dz, *ref["dz"], "bn.dz", dtype)


DGRAD = [k for k in sorted(TC.CONV_CASES) if k != "stem" and not k.startswith("split")]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", DGRAD)
def test_dgrad_restatement_passes(name, dtype):
    c = TC.conv_case(name, dtype, "random", addend=True)
    for addend in (None, c["addend"]):
        ref, E = TC.dgrad_reference(c["dz"], c["w"], c["H"], c["W"], c["stride"], c["pad"], addend)
        got = TC.dgrad_emulate(c["dz"], c["w"], c["H"], c["W"], c["stride"], c["pad"], addend)
        assert TC.check(name, got, ref, E, "dgrad", dtype) <= 1.0
    if name == "1x1-s2":
        ref, E = TC.dgrad_reference(c["dz"], c["w"], c["H"], c["W"], c["stride"], c["pad"])
        assert bool((E[:, 1::2] == 0).all()) and bool((E[:, :, 1::2] == 0).all()) and bool((E[:, ::2, ::2] > 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name,mistake", [("3x3", "flipped-tap"), ("3x3-s2-odd", "flipped-tap"), ("3x3-s2-odd", "wrong-parity"),
                                          ("3x3-s2-even", "wrong-parity"), ("1x1-s2", "wrong-parity")])
def test_dgrad_rejects_mistakes(name, mistake, dtype):
    c = TC.conv_case(name, dtype, "random")
    ref, E = TC.dgrad_reference(c["dz"], c["w"], c["H"], c["W"], c["stride"], c["pad"])
    bad = TC.dgrad_emulate(c["dz"], c["w"], c["H"], c["W"], c["stride"], c["pad"], mistake=mistake)
    with pytest.raises(AssertionError):
        TC.check(name, bad, ref, E, "dgrad", dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(TC.CONV_CASES))
def test_wgrad_restatement_passes(name, dtype):
    c = TC.conv_case(name, dtype, "random")
    ref, E = TC.wgrad_reference(c["dz"], c["x"], c["R"], c["stride"], c["pad"])
    got = TC.wgrad_emulate(c["dz"], c["x"], c["R"], c["stride"], c["pad"])
    assert TC.check(name, got, ref, E, "wgrad", dtype) <= 1.0
    if name == "stem":
        assert bool((E[..., 3:] == 0).all()) and bool((E[..., :3] > 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["split-1x1", "split-3x3"])
def test_wgrad_rejects_a_dropped_split(name, dtype):
    c = TC.conv_case(name, dtype, "random")
    ref, E = TC.wgrad_reference(c["dz"], c["x"], c["R"], c["stride"], c["pad"])
    bad = TC.wgrad_emulate(c["dz"], c["x"], c["R"], c["stride"], c["pad"], mistake="split-dropped")
    with pytest.raises(AssertionError):
        TC.check(name, bad, ref, E, "wgrad", dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("family", ["exact"])
def test_exact_family_is_exact(dtype, family):
    c = TC.conv_case("3x3-s2-odd", dtype, family, addend=True)
    ref, E = TC.dgrad_reference(c["dz"], c["w"], c["H"], c["W"], c["stride"], c["pad"], c["addend"])
    TC.exact_sum_bound(ref, E)
    TC.check_exact("dgrad", TC.dgrad_emulate(c["dz"], c["w"], c["H"], c["W"], c["stride"], c["pad"], c["addend"]), ref)
    bad = TC.dgrad_emulate(c["dz"], c["w"], c["H"], c["W"], c["stride"], c["pad"], c["addend"], mistake="flipped-tap")
    with pytest.raises(AssertionError):
        TC.check_exact("dgrad", bad, ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("H", [7, 8])
def test_maxpool_backward_first_maximum(H, dtype):
    g = torch.Generator().manual_seed(H)
    dy = torch.randn(2, 4, 4, 8, generator=g).to(dtype)
    zeros = torch.zeros(2, H, H, 8, dtype=dtype)
    ref, E = TC.maxpool_bwd_reference(zeros, dy)
    # ties everywhere: the first real tap of window ho is in row 2 ho - 1, or row 0 for ho = 0, so rows 2, 4, 6 win nothing
    assert bool((E[:, 2::2] == 0).all()) and bool((E[:, :, 2::2] == 0).all()) and bool((E[:, 0, 0] > 0).all())
    last, _ = TC.maxpool_bwd_reference(zeros, dy, last=True)
    assert TC.check("first", ref.to(dtype), ref, E, "pool.dx", dtype) <= 1.0
    with pytest.raises(AssertionError):
        TC.check("last", last.to(dtype), ref, E, "pool.dx", dtype)
    x = torch.randperm(2 * H * H * 8, generator=g).float().reshape(2, H, H, 8).to(torch.float32)      # distinct values
    ref, E = TC.maxpool_bwd_reference(x, dy.float())
    xa = x.clone().requires_grad_(True)
    torch.nn.functional.max_pool2d(xa.permute(0, 3, 1, 2), 3, 2, 1).backward(dy.float().permute(0, 3, 1, 2))
    assert TC.check("torch", xa.grad, ref, E, "pool.dx", torch.float32) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode,idx", [(0, [0, 1, 2]), (1, [2, 0])])
def test_gate_gradient_restatement(mode, idx, dtype):
    g = torch.Generator().manual_seed(mode)
    E_, n, L = 3, 2, 257 * 8
    X = torch.randn(E_, n, L, generator=g).to(dtype)
    dout = torch.randn((n, L) if mode == 0 else (n, len(idx), L), generator=g).to(dtype)
    gate = torch.softmax(torch.randn(n, E_, generator=g), -1)
    ref, E = TC.gate_bwd_reference(X, dout, gate, idx, mode)
    assert TC.check("dgate", TC.gate_bwd_emulate(X, dout, gate, idx, mode), ref, E, "dgate", dtype, U32) <= 1.0
    if mode == 1:
        assert bool((E[:, 1] == 0).all()) and bool((ref[:, 1] == 0).all())            # the unlisted expert
        plain = TC.gate_bwd_emulate(X, dout, gate, idx, 1, mistake="no-softmax-bwd")
        with pytest.raises(AssertionError):
            TC.check("dgate", plain, ref, E, "dgate", dtype, U32)
