"""Self-test of the convolution checker (tests/conv_check.py) on the CPU: it accepts a correctly rounded result and REJECTS the
mistakes an implicit-GEMM convolution kernel makes -- two output channels swapped, a padding that is off by one, a missing ReLU, a
residual that was not added, a value written past the output -- each produced by corrupting the fp64 reference, in both storage
types and at the bound's constant c = 1 and 8 (the constants in use are at most 2)."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_check as CC
from tests.kernel_check import Guarded, U

DTYPES = [torch.bfloat16, torch.float32]


def _case(dtype, family="random"):
    return CC.make_case(2, 9, 7, 64, 64, 3, 1, 1, True, True, dtype, family, seed=11)


def _ref(case, **over):
    a = dict(case)
    a.update(over)
    return CC.reference(a["x"], a["w"], a["scale"], a["shift"], a["residual"], a["relu"], a["stride"], a["pad"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_accepts_a_correctly_rounded_result(dtype):
    case = _case(dtype)
    ref, E, _ = _ref(case)
    assert CC.check("ok", ref.to(dtype), ref, E, 1.0, U[dtype]) <= 1.0
    ex = _case(dtype, "exact")
    r = CC.exact_reference(ex["x"], ex["w"], ex["scale"], ex["shift"], ex["residual"], ex["relu"], ex["stride"], ex["pad"])
    CC.check_exact("ok", r.float().to(dtype), r)


@pytest.mark.parametrize("c", [1.0, 8.0])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("mistake", ["channels-swapped", "padding-off-by-one", "no-relu", "no-residual"])
def test_rejects_kernel_mistakes(mistake, dtype, c):
    case = _case(dtype)
    ref, E, _ = _ref(case)
    if mistake == "channels-swapped":
        bad = ref.clone()
        bad[..., [5, 6]] = ref[..., [6, 5]]
    elif mistake == "padding-off-by-one":      # the window shifted by one pixel: what pad = 0 on a pre-padded image of pad 2 computes
        xp = F.pad(case["x"].double().permute(0, 3, 1, 2), (2, 2, 2, 2))[:, :, :-2, :-2].permute(0, 2, 3, 1)
        bad, _, _ = CC.reference(xp.to(dtype), case["w"], case["scale"], case["shift"], case["residual"], case["relu"], 1, 0)
    elif mistake == "no-relu":
        bad, _, _ = _ref(case, relu=False)
    else:
        bad, _, _ = _ref(case, residual=None)
    assert bad.shape == ref.shape
    with pytest.raises(AssertionError):
        CC.check(mistake, bad.to(dtype), ref, E, c, U[dtype])
    exc = _case(dtype, "exact")
    r = CC.exact_reference(exc["x"], exc["w"], exc["scale"], exc["shift"], exc["residual"], exc["relu"], 1, 1)
    if mistake == "channels-swapped":
        b = r.clone()
        b[..., [5, 6]] = r[..., [6, 5]]
    elif mistake == "padding-off-by-one":
        xp = F.pad(exc["x"].double().permute(0, 3, 1, 2), (2, 2, 2, 2))[:, :, :-2, :-2].permute(0, 2, 3, 1)
        b, _, _ = CC.reference(xp.to(dtype), exc["w"], exc["scale"], exc["shift"], exc["residual"], exc["relu"], 1, 0)
    elif mistake == "no-relu":
        b, _, _ = _ref(exc, relu=False)
    else:
        b, _, _ = _ref(exc, residual=None)
    with pytest.raises(AssertionError):
        CC.check_exact(mistake, b.float().to(dtype), r)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_rejects_a_write_past_the_output(dtype):
    gd = Guarded(2 * 9 * 7 * 64, dtype, "cpu")
    y = gd.view((2, 9, 7, 64), (9 * 7 * 64, 7 * 64, 64, 1))
    y.zero_()
    gd.verify("y")
    gd.buf[gd.pad + y.numel()] = 1.0            # one element past the last pixel: a ragged tile stored unmasked
    with pytest.raises(AssertionError, match="outside the output"):
        gd.verify("y")
    gd2 = Guarded(64, dtype, "cpu")
    gd2.view((64,), (1,))[:63] = 0
    with pytest.raises(AssertionError, match="never written"):
        gd2.verify("y")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_head_checker(dtype):
    g = torch.Generator().manual_seed(5)
    x = torch.relu(torch.randn(3, 6, 2048, generator=g)).to(dtype)
    w = (torch.randn(5, 2048, generator=g) * 2048 ** -0.5).to(dtype)
    b = (4.0 * torch.arange(5).float()).to(dtype)
    ref = CC.head_reference(x, w, b, 5)
    assert CC.check("logits", ref["logits"].to(dtype), ref["logits"], ref["E_logits"], 1.0, U[dtype]) <= 1.0
    assert ref["topk"].tolist() == [[4, 3, 2, 1, 0]] * 3
    wrong = ref["logits"].clone()
    wrong[:, 0] += 4 * U[dtype] * ref["E_logits"][:, 0]
    with pytest.raises(AssertionError):
        CC.check("logits", wrong, ref["logits"], ref["E_logits"], 2.0, U[dtype])
    p_of_unrounded = torch.softmax(ref["logits"], -1)
    assert CC.check("weights", torch.softmax(ref["logits"].to(dtype).double(), -1).to(dtype), p_of_unrounded, ref["E_weights"], 1.0,
                    U[dtype]) <= 1.0
