"""functional.grouped_linear / grouped_layernorm against E calls of functional.linear / layernorm on the row slices, BIT FOR BIT:
outputs, dx and every parameter's `.grad`, with the experts trained in step (one batched gradient write) and out of step (some
frozen, or disagreeing on overwrite versus accumulate: the per-expert fallbacks of GroupedLinearFn / GroupedLayerNormFn.backward).
None of these kernels sums with atomics, so there is no tolerance anywhere in this file.

E = 3 experts of R = 40 rows each: above the M <= 16 cut-off under which the batched GEMM wrapper loops mm_gemm, and no multiple of
any tile."""
import pytest
import torch

pytestmark = pytest.mark.gpu

E, R = 3, 40
CASES = ["all_fresh", "expert1_frozen", "expert1_half_frozen", "expert2_accumulates", "all_accumulate"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _params(shapes, dtype, gen, case, half):
    """-> per expert a dict name -> (value, requires_grad, the gradient it already holds or None).  `half`: the one parameter of
    expert 1 that `expert1_half_frozen` freezes."""
    out = []
    for e in range(E):
        d = {}
        for name, shape in shapes.items():
            val = (torch.randn(shape, generator=gen) * 0.5 + (1.0 if name == "ln_w" else 0.0)).to(dtype).cuda()
            frozen = e == 1 and (case == "expert1_frozen" or (case == "expert1_half_frozen" and name == half))
            holds = case == "all_accumulate" or (case == "expert2_accumulates" and e == 2)
            old = torch.randn(shape, generator=gen).to(dtype).cuda() if holds and not frozen else None
            d[name] = (val, not frozen, old)
        out.append(d)
    return out


def _clone(spec):
    """fresh Parameters of one side: the same values, the same flags, a copy of the same earlier gradient"""
    ps = []
    for d in spec:
        q = {}
        for name, (val, req, old) in d.items():
            p = torch.nn.Parameter(val.clone(), requires_grad=req)
            if old is not None:
                p.grad = old.clone()
            q[name] = p
        ps.append(q)
    return ps


def _spied(fn, params):
    """run fn under a gradient-ready spy -> the (expert, name) of every parameter it saw, in order; the earlier hook comes back"""
    from multimeditron_amd import functional as Fm
    who = {id(p): (e, name) for e, q in enumerate(params) for name, p in q.items()}
    seen, before = [], Fm._grad_ready_hook
    Fm.set_grad_ready_hook(lambda p: seen.append(who[id(p)]))
    try:
        fn()
    finally:
        Fm.set_grad_ready_hook(before)
    torch.cuda.synchronize()
    return seen


def _check_params(spec, grouped, single, seen_g, seen_s, ops):
    """every `.grad` bit for bit; the ready hook once per trainable parameter, in the order of the per-expert calls taken expert by
    expert within one op (`ops`: the parameter names each gradient launch of the grouped Function writes, in its launch order)"""
    trainable = [(e, name) for e, d in enumerate(spec) for name, (_, req, _) in d.items() if req]
    for e, d in enumerate(spec):
        for name, (_, req, _) in d.items():
            g, s = grouped[e][name].grad, single[e][name].grad
            if not req:
                assert g is None and s is None, (e, name)
            else:
                assert g is not None and s is not None and torch.equal(g, s), (e, name, float((g.float() - s.float()).abs().max()))
    assert sorted(seen_s) == sorted(trainable) and sorted(seen_g) == sorted(trainable), (seen_g, seen_s)
    assert seen_g == [k for op in ops for k in seen_s if k[1] in op], (seen_g, seen_s)
    assert not torch.equal(grouped[0][ops[0][0]].grad, grouped[2][ops[0][0]].grad)       # the experts really differ


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("epilogue", ["plain", "quick_gelu+residual"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_grouped_linear_equals_per_expert_linear(dtype, epilogue, case):
    from multimeditron_amd import functional as Fm
    from multimeditron_amd._lib import EPI_QUICK_GELU
    from multimeditron_amd.nn import grad_dummy
    K, N = 64, 96
    gen = torch.Generator().manual_seed(21)
    rnd = lambda *s: (torch.randn(s, generator=gen) * 0.5).to(dtype).cuda()
    x, dy = rnd(E * R, K), rnd(E * R, N)
    fancy = epilogue != "plain"
    res = rnd(E * R, N) if fancy else None
    act = EPI_QUICK_GELU if fancy else 0
    spec = _params({"w": (N, K), "b": (N,)}, dtype, gen, case, half="b")
    grouped, single = _clone(spec), _clone(spec)
    rows = [slice(e * R, (e + 1) * R) for e in range(E)]

    xg = x.clone().requires_grad_()
    rg = res.clone().requires_grad_() if fancy else None
    yg = Fm.grouped_linear(xg, [q["w"] for q in grouped], [q["b"] for q in grouped], residual=rg, act=act,
                           dummy=grad_dummy(grouped[0]["w"]))
    seen_g = _spied(lambda: yg.backward(dy), grouped)

    xs = [x[sl].clone().requires_grad_() for sl in rows]
    rs = [res[sl].clone().requires_grad_() for sl in rows] if fancy else [None] * E
    ys = [Fm.linear(xs[e], single[e]["w"], single[e]["b"], residual=rs[e], act=act, dummy=grad_dummy(single[e]["w"])) for e in range(E)]
    seen_s = _spied(lambda: [ys[e].backward(dy[rows[e]]) for e in range(E)], single)        # expert by expert

    assert torch.equal(yg, torch.cat(ys))
    assert torch.equal(xg.grad, torch.cat([t.grad for t in xs]))
    if fancy:
        assert torch.equal(rg.grad, torch.cat([t.grad for t in rs]))
    _check_params(spec, grouped, single, seen_g, seen_s, ops=(("b",), ("w",)))        # the column sums, then the weight gradients


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("with_dres", [False, True], ids=["no-dres", "dres"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_grouped_layernorm_equals_per_expert_layernorm(dtype, with_dres, case):
    from multimeditron_amd import functional as Fm
    from multimeditron_amd.nn import grad_dummy
    H, eps = 128, 1e-5
    gen = torch.Generator().manual_seed(22)
    rnd = lambda *s: torch.randn(s, generator=gen).to(dtype).cuda()
    x, dy, dres = rnd(E * R, H), rnd(E * R, H), rnd(E * R, H)
    spec = _params({"ln_w": (H,), "ln_b": (H,)}, dtype, gen, case, half="ln_w")
    grouped, single = _clone(spec), _clone(spec)
    rows = [slice(e * R, (e + 1) * R) for e in range(E)]

    xg = x.clone().requires_grad_()
    yg, xres_g = Fm.grouped_layernorm(xg, [q["ln_w"] for q in grouped], [q["ln_b"] for q in grouped], eps,
                                      dummy=grad_dummy(grouped[0]["ln_w"]))
    outs, grads = ([yg, xres_g], [dy, dres]) if with_dres else ([yg], [dy])
    seen_g = _spied(lambda: torch.autograd.backward(outs, grads), grouped)

    xs = [x[sl].clone().requires_grad_() for sl in rows]
    pairs = [Fm.layernorm(xs[e], single[e]["ln_w"], single[e]["ln_b"], eps, dummy=grad_dummy(single[e]["ln_w"])) for e in range(E)]

    def per_expert():
        for e, sl in enumerate(rows):
            torch.autograd.backward(list(pairs[e]) if with_dres else [pairs[e][0]], [dy[sl], dres[sl]] if with_dres else [dy[sl]])

    seen_s = _spied(per_expert, single)

    assert torch.equal(yg, torch.cat([y for y, _ in pairs]))
    assert torch.equal(xres_g, torch.cat([r for _, r in pairs]))
    assert torch.equal(xg.grad, torch.cat([t.grad for t in xs]))
    _check_params(spec, grouped, single, seen_g, seen_s, ops=(("ln_w", "ln_b"),))      # one launch writes a norm's weight and bias
