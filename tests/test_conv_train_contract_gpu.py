"""The kernels that train the MoE gate (csrc/mm_conv_bwd.hip, mm_expert_fuse_gate_bwd) against their contracts (include/mm_hip.h),
on the GPU: the smallest shapes at which each path can still go wrong, bf16 and f32, every output in a NaN-sentinel guarded
storage, every launch made twice and compared bit for bit, every result held to the fp64 bound of tests/conv_train_check.py
(c = 2) or, in the exact families and wherever the error scale is 0, to equality."""
import pytest
import torch

from tests import conv_train_check as TC
from tests.kernel_check import U32, check_bits, verify_guards

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
IDS = ["bf16", "f32"]
DGRAD = [k for k in sorted(TC.CONV_CASES) if k != "stem" and not k.startswith("split")]


def _twice(run):
    """run() -> (outputs, guards); launched twice into fresh guarded storages: same bits, guards intact"""
    a, ga = run()
    b, gb = run()
    torch.cuda.synchronize()
    verify_guards(ga)
    verify_guards(gb)
    for (name, *_), x, y in zip(ga, a, b):
        check_bits(f"{name}: second launch", y, x)
    return a


# ---- convolution gradients -----------------------------------------------------------------------------------------------------------
def _run_dgrad(c, addend):
    from multimeditron_amd import kernels as K
    wp = c["w"].permute(3, 1, 2, 0).contiguous()                         # [Cin, R, S, Cout]
    n = c["dz"].shape[0]

    def run():
        dx, gd = TC.guarded((n, c["H"], c["W"], wp.shape[0]), c["dz"].dtype, "cuda")
        K.conv2d_nhwc_dgrad(c["dz"], wp, c["H"], c["W"], c["stride"], c["pad"], addend=addend, out=dx)
        return [dx], [("dgrad dx", gd)]
    return _twice(run)[0]


def _run_wgrad(c):
    from multimeditron_amd import kernels as K
    n, H, W, Cin = c["x"].shape
    Cout, R = c["dz"].shape[3], c["R"]
    nbytes = K.conv2d_nhwc_wgrad_ws_bytes(n, H, W, Cin, Cout, R, c["stride"], c["pad"])

    def run():
        dw, gd = TC.guarded((Cout, R, R, Cin), c["x"].dtype, "cuda")
        ws, gw = TC.guarded((nbytes // 4,), torch.float32, "cuda")
        K.conv2d_nhwc_wgrad(c["dz"], c["x"], R, c["stride"], c["pad"], out=dw, ws=ws)
        return [dw, ws], [("wgrad dw", gd), ("wgrad workspace", gw)]
    return _twice(run), nbytes


@pytest.mark.parametrize("addend", [False, True], ids=["plain", "addend"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", DGRAD)
def test_dgrad_random_family(name, dtype, addend):
    c = TC.conv_case(name, dtype, "random", "cuda", addend=addend)
    ref, E = TC.dgrad_reference(c["dz"], c["w"], c["H"], c["W"], c["stride"], c["pad"], c["addend"])
    TC.check(f"dgrad {name}", _run_dgrad(c, c["addend"]), ref, E, "dgrad", dtype)


@pytest.mark.parametrize("addend", [False, True], ids=["plain", "addend"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", DGRAD)
def test_dgrad_exact_family(name, dtype, addend):
    c = TC.conv_case(name, dtype, "exact", "cuda", addend=addend)
    ref, E = TC.dgrad_reference(c["dz"], c["w"], c["H"], c["W"], c["stride"], c["pad"], c["addend"])
    TC.exact_sum_bound(ref, E)
    TC.check_exact(f"dgrad {name}", _run_dgrad(c, c["addend"]), ref)


def test_dgrad_rejects_the_stem():
    from multimeditron_amd import _lib
    from multimeditron_amd import kernels as K
    dz = torch.zeros(1, 9, 9, 64, dtype=torch.bfloat16, device="cuda")
    wp = torch.zeros(64, 7, 7, 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_lib.MMHipError, match="-3"):
        K.conv2d_nhwc_dgrad(dz, wp, 18, 18, 2, 3)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(TC.CONV_CASES))
def test_wgrad_random_family(name, dtype):
    c = TC.conv_case(name, dtype, "random", "cuda")
    ref, E = TC.wgrad_reference(c["dz"], c["x"], c["R"], c["stride"], c["pad"])
    (dw, _), nbytes = _run_wgrad(c)
    TC.check(f"wgrad {name}", dw, ref, E, "wgrad", dtype)
    n, Ho, Wo, Cout = c["dz"].shape
    splits = nbytes // (4 * Cout * c["R"] ** 2 * c["x"].shape[3])
    assert splits == -(-n * Ho * Wo // TC.WGRAD_ROWS)
    if name.startswith("split"):
        assert splits == 3                                               # more than one M split, through the workspace query
    if name == "stem":
        assert bool((dw[..., 3:].float() == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(TC.CONV_CASES))
def test_wgrad_exact_family(name, dtype):
    c = TC.conv_case(name, dtype, "exact", "cuda")
    ref, E = TC.wgrad_reference(c["dz"], c["x"], c["R"], c["stride"], c["pad"])
    TC.exact_sum_bound(ref, E)
    (dw, _), _ = _run_wgrad(c)
    TC.check_exact(f"wgrad {name}", dw, ref)


# ---- BatchNorm -----------------------------------------------------------------------------------------------------------------------
def _run_bn_fwd(case, calls=1):
    from multimeditron_amd import kernels as K
    z = case["z"]
    M, C = z.shape

    def run():
        y, gy = TC.guarded((M, C), z.dtype, "cuda")
        mean, gm = TC.guarded((C,), torch.float32, "cuda")
        invstd, gi = TC.guarded((C,), torch.float32, "cuda")
        ws, gw = TC.guarded((K.bn_train_ws(M, C, "cuda").numel(),), torch.float32, "cuda")
        rm, grm = TC.guarded((C,), z.dtype, "cuda")
        rv, grv = TC.guarded((C,), z.dtype, "cuda")
        rm.copy_(case["running_mean"])
        rv.copy_(case["running_var"])
        nbt = case["num_batches_tracked"].clone()
        for _ in range(calls):
            K.bn_train_fwd(z, case["gamma"], case["beta"], case["residual"], case["relu"], running_mean=rm, running_var=rv,
                           num_batches_tracked=nbt, out=y, mean=mean, invstd=invstd, ws=ws)
        return [y, mean, invstd, rm, rv, nbt.view(1).to(torch.float32)], [("bn y", gy), ("bn mean", gm), ("bn invstd", gi), ("bn rm", grm),
                                                                          ("bn rv", grv)] + [("bn ws", gw, False)]
    return _twice(run)


BN_SHAPES = [(2, 64), (33, 64), (4099, 64), (33, 2048)]


@pytest.mark.parametrize("residual,relu", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["plain", "res", "relu", "res-relu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,C", BN_SHAPES)
def test_bn_train_forward(M, C, dtype, residual, relu):
    case = TC.bn_case(M, C, dtype, residual, relu, seed=M + C, device="cuda")
    ref = TC.bn_fwd_reference(case["z"], case["gamma"], case["beta"], case["residual"], relu)
    y, mean, invstd, rm, rv, nbt = _run_bn_fwd(case)
    TC.check("mean", mean, *ref["mean"], "bn.mean", dtype, U32)
    TC.check("invstd", invstd, *ref["invstd"], "bn.invstd", dtype, U32)
    TC.check("y", y, *ref["y"], "bn.y", dtype)
    TC.check("running_mean", rm, *TC.bn_running_reference(case["running_mean"], *ref["mean"]), "bn.running_mean", dtype)
    TC.check("running_var", rv, *TC.bn_running_reference(case["running_var"], *ref["unbiased"]), "bn.running_var", dtype)
    assert int(nbt) == 8
    assert float(ref["var"][0][0]) == 0.0                                # the constant channel: invstd = eps^-1/2 within its bound


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bn_running_statistics_after_two_calls(dtype):
    case = TC.bn_case(33, 64, dtype, False, False, seed=5, device="cuda")
    ref = TC.bn_fwd_reference(case["z"], case["gamma"], case["beta"], None, False)
    _, _, _, rm, rv, nbt = _run_bn_fwd(case, calls=2)
    for name, start, (b, Eb), got in (("running_mean", case["running_mean"], ref["mean"], rm),
                                      ("running_var", case["running_var"], ref["unbiased"], rv)):
        r1, E1 = TC.bn_running_reference(start, b, Eb)
        # the second update reads the ROUNDED first one: its own rounding plus the first's error carried through the factor 0.9
        first = r1.to(dtype)
        r2, E2 = TC.bn_running_reference(first, b, Eb)
        bad = (first.double() - r1).abs() > 2 * TC.U[dtype] * E1
        assert not bool(bad.any())
        r2_exact = 0.9 * r1 + 0.1 * b
        TC.check(name, got, r2_exact, E2 + 0.9 * 2 * E1, "bn." + name, dtype)
    assert int(nbt) == 9


def test_bn_rejects_a_single_row():
    from multimeditron_amd import _lib
    L = _lib.lib()
    z = torch.zeros(1, 64, device="cuda")
    v = torch.zeros(64, device="cuda")
    ws = torch.zeros(1024, device="cuda")
    p = lambda t: t.data_ptr()
    assert L.mm_bn_train_fwd(1, p(z), 1, 64, p(v), p(v), None, 0, 1e-5, 0.1, p(z), p(v), p(v), None, None, None, p(ws), 4096, None) == -1
    assert L.mm_bn_train_bwd(1, p(z), p(z), p(z), 1, 64, p(v), p(v), p(v), 0, p(z), None, p(v), p(v), p(ws), 4096, None) == -1


@pytest.mark.parametrize("residual,relu", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["plain", "res", "relu", "res-relu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,C", BN_SHAPES)
def test_bn_train_backward(M, C, dtype, residual, relu):
    from multimeditron_amd import kernels as K
    case = TC.bn_case(M, C, dtype, residual, relu, seed=M + C + 1, device="cuda")
    y, mean, invstd = K.bn_train_fwd(case["z"], case["gamma"], case["beta"], case["residual"], relu)
    ref = TC.bn_bwd_reference(case["dy"], y, case["z"], mean, invstd, case["gamma"], relu)

    def run():
        dz, g1 = TC.guarded((M, C), dtype, "cuda")
        dres, g2 = TC.guarded((M, C), dtype, "cuda") if residual else (None, None)
        dgamma, g3 = TC.guarded((C,), dtype, "cuda")
        dbeta, g4 = TC.guarded((C,), dtype, "cuda")
        ws, g5 = TC.guarded((K.bn_train_ws(M, C, "cuda").numel(),), torch.float32, "cuda")
        K.bn_train_bwd(case["dy"], y, case["z"], mean, invstd, case["gamma"], relu, dz=dz, dres=dres, dgamma=dgamma, dbeta=dbeta, ws=ws)
        outs, guards = [dz, dgamma, dbeta, ws], [("bn dz", g1), ("bn dgamma", g3), ("bn dbeta", g4), ("bn bwd ws", g5)]
        if residual:
            outs.append(dres)
            guards.append(("bn dres", g2))
        return outs, guards
    out = _twice(run)
    TC.check("dz", out[0], *ref["dz"], "bn.dz", dtype)
    TC.check("dgamma", out[1], *ref["dgamma"], "bn.dgamma", dtype)
    TC.check("dbeta", out[2], *ref["dbeta"], "bn.dbeta", dtype)
    if residual:
        TC.check("dres", out[4], *ref["dres"], "bn.dres", dtype)          # E = 0: the bits of dy or zero


# ---- max-pool backward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["zeros", "distinct", "relu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("H", [7, 8])
def test_maxpool_backward(H, dtype, kind):
    from multimeditron_amd import kernels as K
    g = torch.Generator().manual_seed(H)
    if kind == "zeros":
        x = torch.zeros(2, H, H, 8)
    elif kind == "distinct":
        x = (torch.randperm(2 * H * H * 8, generator=g).float().reshape(2, H, H, 8) - 400.0) / 4      # exact in bf16, mostly negative
    else:
        x = torch.relu(torch.randn(2, H, H, 8, generator=g))              # post-ReLU: zeros tie, positive values do not
    x = x.to(dtype).cuda()
    dy = torch.randn(2, 4, 4, 8, generator=g).to(dtype).cuda()
    ref, E = TC.maxpool_bwd_reference(x, dy)

    def run():
        dx, gd = TC.guarded((2, H, H, 8), dtype, "cuda")
        K.maxpool2d_nhwc_bwd(x, dy, out=dx)
        return [dx], [("pool dx", gd)]
    dx = _twice(run)[0]
    TC.check(f"pool {kind}", dx, ref, E, "pool.dx", dtype)
    if kind != "zeros":              # torch's CPU backward (its rule is the first maximal element; all-equal windows are left to the rule above)
        xa = x.float().cpu().requires_grad_(True)
        torch.nn.functional.max_pool2d(xa.permute(0, 3, 1, 2), 3, 2, 1).backward(dy.float().cpu().permute(0, 3, 1, 2))
        TC.check(f"pool {kind} vs torch", dx, xa.grad.double().cuda(), E, "pool.dx", dtype)


# ---- the gate's gradient through the fusion ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["random", "exact"])
@pytest.mark.parametrize("mode,idx", [(0, [0, 1, 2]), (1, [2, 0])], ids=["average-all", "softmax-two-of-three"])
@pytest.mark.parametrize("L", [128, 257 * 8])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_expert_fuse_gate_bwd(dtype, L, mode, idx, family):
    from multimeditron_amd import kernels as K
    g = torch.Generator().manual_seed(L + mode)
    E_, n, J = 3, 2, len(idx)
    if family == "exact":                                                 # integers; equal gate weights make the softmax exactly 1/2
        X = torch.randint(-4, 5, (E_, n, L), generator=g).float()
        dout = torch.randint(-4, 5, (n, L) if mode == 0 else (n, J, L), generator=g).float()
        gate = torch.full((n, E_), 0.25)
    else:
        X = torch.randn(E_, n, L, generator=g)
        dout = torch.randn((n, L) if mode == 0 else (n, J, L), generator=g)
        gate = torch.softmax(torch.randn(n, E_, generator=g), -1)
    X, dout, gate = X.to(dtype).cuda(), dout.to(dtype).cuda(), gate.cuda()
    ref, E = TC.gate_bwd_reference(X, dout, gate, idx, mode)

    def run():
        dg, gd = TC.guarded((n, E_), torch.float32, "cuda")
        K.expert_fuse_gate_bwd(X, dout, gate, idx, mode, out=dg)
        return [dg], [("dgate", gd)]
    dg = _twice(run)[0]
    if family == "exact":
        assert 16 * L < 2 ** 24                                            # every partial sum is an integer fp32 holds
        check_bits("dgate exact", dg, ref.float(), zero_sign=False)
    else:
        TC.check("dgate", dg, ref, E, "dgate", dtype, U32)
    if mode == 1:
        assert bool((dg[:, 1] == 0).all())                                # the unlisted expert


@pytest.mark.parametrize("mode,idx", [(0, [0, 1, 2]), (1, [1, 2])])
def test_expert_fuse_gives_the_gate_a_gradient(mode, idx):
    """the autograd function: dgate only when the gate asks for it, the experts' gradient unchanged bit for bit"""
    from multimeditron_amd import functional as Fm
    g = torch.Generator().manual_seed(9)
    x = torch.randn(3, 2, 5, 16, generator=g).to(torch.bfloat16).cuda()
    gate = torch.softmax(torch.randn(2, 3, generator=g), -1).cuda()
    outs = []
    for want in (False, True):
        xa, ga = x.clone().requires_grad_(True), gate.clone().requires_grad_(want)
        out = Fm.expert_fuse(xa, ga, idx, mode)
        dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).cuda()
        out.backward(dout)
        outs.append((out.detach(), xa.grad, ga.grad))
    assert outs[0][2] is None and outs[1][2] is not None and outs[1][2].dtype == torch.float32
    check_bits("out", outs[1][0], outs[0][0])
    check_bits("dx", outs[1][1], outs[0][1])
    L = 5 * 16
    d = dout.view(2, L) if mode == 0 else dout.view(2, len(idx), L)
    ref, E = TC.gate_bwd_reference(x.view(3, 2, L), d, gate, idx, mode)
    TC.check("dgate", outs[1][2], ref, E, "dgate", torch.bfloat16, U32)
