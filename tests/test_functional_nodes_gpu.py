"""The fused autograd nodes of functional.py against the nodes they stand for, BIT FOR BIT: outputs, input gradients, every
parameter's `.grad` and the order of the gradient-ready calls (as tests/test_grouped_autograd_gpu.py does for the grouped nodes).

    qkv_rope_attention                    =  linear -> rope_attention
    swiglu_mlp                            =  linear -> swiglu -> linear(residual=)
    linear(act=GELU, residual=)           =  linear -> mm_gelu_fwd -> mm_add, backward through mm_gelu_bwd

The right-hand sides run the separate launches; the left-hand sides take the fused ones where a shape qualifies (mm_gemm_rope_fwd,
mm_gemm_swiglu_fwd / _bwd, mm_gemm_act_fwd), which tests/test_kernels_gpu.py holds to the same bits launch by launch.  Both sides
share one projection backward (column sums, weight gradient, input gradient), which is what this file watches: with fresh, frozen
and accumulating parameters, and with one parameter of the node frozen alone.  bf16, and fp32 for the SwiGLU node's unfused backward: a width that is no multiple
of 4 (I = 6) cannot stand in for it, because mm_swiglu_fwd / _bwd themselves refuse it (MM_ERR_ALIGN: I % 8 in bf16, I % 4 in fp32),
before and after this file was written.  No fp32 attention case: its backward sums with atomics.  The Qwen3 and xIELU nodes have no composition to stand against; the training
launch trace, test_qk_norm_gpu.py and test_apertus_model_gpu.py hold them."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
CASES = ["fresh", "frozen", "accumulates", "one_frozen"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _spec(shapes, gen, case, alone, dtype=BF):
    """name -> (value, requires_grad, the gradient it already holds or None); `alone`: the parameter `one_frozen` freezes"""
    d = {}
    for name, shape in shapes.items():
        val = (torch.randn(shape, generator=gen) * 0.1).to(dtype).cuda()
        frozen = case == "frozen" or (case == "one_frozen" and name == alone)
        old = torch.randn(shape, generator=gen).to(dtype).cuda() if case == "accumulates" else None
        d[name] = (val, not frozen, old)
    return d


def _clone(spec):
    ps = {}
    for name, (val, req, old) in spec.items():
        p = torch.nn.Parameter(val.clone(), requires_grad=req)
        if old is not None:
            p.grad = old.clone()
        ps[name] = p
    return ps


def _backward(outs, grads, params):
    """backward under a gradient-ready spy -> the names it saw, in order"""
    from multimeditron_amd import functional as Fm
    who = {id(p): name for name, p in params.items()}
    seen, before = [], Fm._grad_ready_hook
    Fm.set_grad_ready_hook(lambda p: seen.append(who[id(p)]))
    try:
        torch.autograd.backward(outs, grads)
    finally:
        Fm.set_grad_ready_hook(before)
    torch.cuda.synchronize()
    return seen


def _check(spec, fused, split, seen_f, seen_s, order):
    for name, (_, req, _) in spec.items():
        f, s = fused[name].grad, split[name].grad
        if not req:
            assert f is None and s is None, name
        else:
            assert f is not None and s is not None and torch.equal(f, s), (name, float((f.float() - s.float()).abs().max()))
            assert bool(f.float().abs().sum() > 0), name
    assert seen_f == seen_s == [n for n in order if n in spec and spec[n][1]], (seen_f, seen_s)


def _dummy(params):
    from multimeditron_amd.nn import grad_dummy
    ps = list(params.values())
    return grad_dummy(next((p for p in ps if p.requires_grad), ps[0]))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", [(2, 40, 4, 2, 64), (1, 256, 2, 1, 128)], ids=["two_launch", "rope_epilogue"])
def test_qkv_rope_attention_equals_linear_then_rope_attention(shape, bias, case):
    from multimeditron_amd import functional as Fm, kernels as K
    B, S, Hq, Hkv, D = shape
    Kd, T, N = 64, B * S, (Hq + 2 * Hkv) * D
    gen = torch.Generator().manual_seed(31)
    rnd = lambda *s: (torch.randn(s, generator=gen) * 0.5).to(BF).cuda()
    h, dout = rnd(T, Kd), rnd(T, Hq * D)
    pos = torch.arange(S, dtype=torch.int64).repeat(B).cuda()
    inv = (1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))).cuda()
    cos, sin = K.rope_table(pos, inv, True)
    assert (K.gemm_rope_fwd(h, rnd(N, Kd), None, (Hq + Hkv) * D, D, cos, sin) is not None) == (D == 128)      # the route the id names
    spec = _spec({"w": (N, Kd), "b": (N,)} if bias else {"w": (N, Kd)}, gen, case, alone="b" if bias else "w")
    fused, split = _clone(spec), _clone(spec)
    args = (cos, sin, None, B, S, Hq, Hkv, D, True, D ** -0.5)

    hf = h.clone().requires_grad_()
    of = Fm.qkv_rope_attention(hf, fused["w"], fused.get("b"), *args, dummy=_dummy(fused))
    seen_f = _backward([of], [dout], fused)

    hs = h.clone().requires_grad_()
    os_ = Fm.rope_attention(Fm.linear(hs, split["w"], split.get("b"), dummy=_dummy(split)), *args)
    seen_s = _backward([os_], [dout], split)

    assert torch.equal(of, os_) and torch.equal(hf.grad, hs.grad)
    _check(spec, fused, split, seen_f, seen_s, order=("b", "w"))            # the column sums, then the weight gradient


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("shape", [(80, 128, BF), (256, 128, BF), (80, 12, torch.float32)], ids=["fused_bwd", "fused_fwd_bwd", "unfused_f32"])
def test_swiglu_mlp_equals_linear_swiglu_linear(shape, case):
    from multimeditron_amd import functional as Fm, kernels as K
    T, I, dtype = shape          # fp32: the route through the separate SwiGLU kernels in forward AND backward
    H = 64
    gen = torch.Generator().manual_seed(32)
    rnd = lambda *s: (torch.randn(s, generator=gen) * 0.5).to(dtype).cuda()
    x, res, dy = rnd(T, H), rnd(T, H), rnd(T, H)
    assert (K.gemm_swiglu_fwd(x, rnd(2 * I, H), I) is not None) == (T >= 256)                                    # the routes the id names
    assert (K.gemm_swiglu_bwd(dy, rnd(H, I), rnd(T, 2 * I), I) is not None) == (dtype == BF)
    spec = _spec({"wgu": (2 * I, H), "wd": (H, I)}, gen, case, alone="wd", dtype=dtype)
    fused, split = _clone(spec), _clone(spec)

    xf, rf = x.clone().requires_grad_(), res.clone().requires_grad_()
    yf = Fm.swiglu_mlp(xf, fused["wgu"], fused["wd"], I, residual=rf, dummy=_dummy(fused))
    seen_f = _backward([yf], [dy], fused)

    xs, rs = x.clone().requires_grad_(), res.clone().requires_grad_()
    act = Fm.swiglu(Fm.linear(xs, split["wgu"], dummy=_dummy(split)), I)
    ys = Fm.linear(act, split["wd"], residual=rs, dummy=_dummy(split))
    seen_s = _backward([ys], [dy], split)

    assert torch.equal(yf, ys) and torch.equal(xf.grad, xs.grad) and torch.equal(rf.grad, rs.grad)
    _check(spec, fused, split, seen_f, seen_s, order=("wd", "wgu"))         # backward meets down_proj first


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("act_name", ["EPI_GELU_ERF", "EPI_QUICK_GELU"])
def test_linear_with_gelu_and_residual_equals_the_three_launches(act_name, case):
    from multimeditron_amd import _lib, functional as Fm, kernels as K
    act = getattr(_lib, act_name)
    T, Kd, N = 80, 64, 96
    gen = torch.Generator().manual_seed(33)
    rnd = lambda *s: (torch.randn(s, generator=gen) * 0.5).to(BF).cuda()
    x, res, dy = rnd(T, Kd), rnd(T, N), rnd(T, N)
    spec = _spec({"w": (N, Kd), "b": (N,)}, gen, case, alone="b")
    fused, split = _clone(spec), _clone(spec)
    assert K.linear_act_fwd(x, fused["w"].data, fused["b"].data, act, res) is not None                         # the one-launch forward

    xf, rf = x.clone().requires_grad_(), res.clone().requires_grad_()
    yf = Fm.linear(xf, fused["w"], fused["b"], residual=rf, act=act, dummy=_dummy(fused))
    seen_f = _backward([yf], [dy], fused)

    xs = x.clone().requires_grad_()
    pre = Fm.linear(xs, split["w"], split["b"], dummy=_dummy(split))
    ys = K.add(K.gelu_fwd(pre.detach(), _lib.GELU_KIND[act]), res)
    seen_s = _backward([pre], [K.gelu_bwd(pre.detach(), dy, _lib.GELU_KIND[act])], split)

    assert torch.equal(yf, ys) and torch.equal(xf.grad, xs.grad) and torch.equal(rf.grad, dy)
    _check(spec, fused, split, seen_f, seen_s, order=("b", "w"))
