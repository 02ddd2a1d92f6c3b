"""Every GEMM launch path held to exact results (tests/gemm_check.py): small-integer operands scaled by a power of two per row /
column, so that every fp32 partial sum is exact and the bf16 output must equal the one RNE rounding of the fp64 product BIT FOR
BIT, element by element.  Operands sit in NaN-filled storages (zeros only in [K, pad8(K)) of a K-contiguous row), outputs in
NaN-sentinel storages whose guards must stay untouched, and every case asserts the kernel id the dispatcher reports
(mm_get_option "gemm_last_kernel").  The persistent kernels also run with gemm_persist = 0 (one tile per workgroup, no
half-tile round: the trainer's data-parallel mode and the deferred weight gradients), bit-identical to the persistent run.

CASES is the coverage list: tests/test_gemm_check_cpu.py checks that every path meets every edge class (layout, epilogue, N % 8,
K class, grid shape) at least once."""
import math

import pytest
import torch

from tests import gemm_check as GC
from tests.gemm_check import NN, NT, TN
from tests.kernel_check import dt, options, ptr, stream

pytestmark = pytest.mark.gpu

LAYOUT_NAME = {NT: "NT", NN: "NN", TN: "TN"}
EPIS = {"plain": 0, "bias": GC.EPI_BIAS, "residual": GC.EPI_RESIDUAL, "accumulate": GC.EPI_ACCUMULATE,
        "bias+residual": GC.EPI_BIAS | GC.EPI_RESIDUAL, "erf": GC.EPI_GELU_ERF | GC.EPI_BIAS, "quick": GC.EPI_QUICK_GELU,
        "tanh": GC.EPI_GELU_TANH | GC.EPI_RESIDUAL}
ACT_EPIS = ("erf", "quick", "tanh")
TILE = {GC.V1: (128, 128), GC.DMA256x128: (256, 128), GC.DMA256x256: (256, 256), GC.DMA128: (128, 128),
        GC.DMA64x128: (64, 128), GC.DMA64: (64, 64), GC.W4: (256, 256)}
# how each tiled path is forced: gemm_kernel 1 = v1, 2..6 = DMA variants 1..5; the 8-wave 256x256 kernel with gemm_w4 = 0
FORCE = {GC.V1: dict(gemm_kernel=1), GC.DMA256x128: dict(gemm_kernel=2), GC.DMA256x256: dict(gemm_kernel=3, gemm_w4=0),
         GC.DMA128: dict(gemm_kernel=4), GC.DMA64x128: dict(gemm_kernel=5), GC.DMA64: dict(gemm_kernel=6),
         GC.W4: dict(gemm_kernel=3)}
PERSISTENT = (GC.DMA256x128, GC.DMA256x256, GC.DMA128, GC.DMA64x128, GC.DMA64, GC.W4)


def _tiled_shapes(kid):
    """(M, N, K) per tiled path: single tile, a tail-only grid, one full round plus a <= half-full round, more rounds; every
    N % 8 class and K class (K % 64 == 0, ragged K-step, K % 8 != 0, K < 192 -- the 4-wave kernel takes K >= 192 only)."""
    bm, bn = TILE[kid]
    small = 264 if kid == GC.W4 else 130
    return [(bm - 1, bn, 256), (bm, bn - 4, 200), (2 * bm + 3, 3 * bn - 6, small), (17 * bm - 7, 17 * bn - 4, 203),
            (5 * bm, 4 * bn + 2, 448), (bm + 16, 2 * bn, 1000), (3 * bm, bn + 4, 72 if kid != GC.W4 else 192)]


def _cycle(kid, epis, layouts=(NT, NN, TN), opts=None, shapes=None, tag=""):
    shapes = shapes or _tiled_shapes(kid)
    out = []
    n = max(len(shapes), len(epis), len(layouts))
    for i in range(n):
        M, N, K = shapes[i % len(shapes)]
        epi = epis[i % len(epis)]
        lay = layouts[i % len(layouts)] if epi not in ACT_EPIS else NT
        place = GC.PLACEMENTS[i % 3]
        if place == "tight" and N % 4:
            place = "pad64"
        out.append(dict(kid=kid, layout=lay, M=M, N=N, K=K, epi=epi, place=place, opts=dict(opts or FORCE.get(kid, {})),
                        tag=tag))
    return out


BASE_EPIS = ["plain", "bias", "residual", "accumulate", "bias+residual"]
CASES = []
for _kid in (GC.V1, GC.DMA256x128, GC.DMA256x256, GC.DMA128, GC.DMA64x128, GC.DMA64):
    CASES += _cycle(_kid, BASE_EPIS + list(ACT_EPIS))
CASES += _cycle(GC.W4, BASE_EPIS)
CASES += [  # the 4-wave kernel's schedules and epilogue forms
    dict(kid=GC.W4, layout=NT, M=520, N=14344, K=256, epi="bias", place="slice", opts=dict(gemm_kernel=3), tag="sched4 (N >= 14336)"),
    dict(kid=GC.W4, layout=NN, M=300, N=1032, K=14400, epi="accumulate", place="pad64", opts=dict(gemm_kernel=3), tag="sched4 (K >= 14336)"),
    dict(kid=GC.W4, layout=NT, M=4345, N=4348, K=256, epi="residual", place="tight", opts=dict(gemm_kernel=3, gemm_w4=6), tag="sched6"),
    dict(kid=GC.W4, layout=NN, M=1000, N=1544, K=320, epi="plain", place="pad64", opts=dict(gemm_kernel=3, gemm_w4=7), tag="sched7"),
    dict(kid=GC.W4, layout=TN, M=1000, N=1544, K=328, epi="bias+residual", place="tight", opts=dict(gemm_kernel=3, gemm_w4_rowmajor=0), tag="rowmajor off"),
    dict(kid=GC.W4, layout=NT, M=2049, N=1032, K=1000, epi="plain", place="pad64", opts=dict(gemm_kernel=3, gemm_w4_shuffle=1), tag="shuffle"),
    # the 8-wave kernel without the half-tile round, and under the default dispatch for K < 192
    dict(kid=GC.DMA256x256, layout=NT, M=4345, N=4348, K=203, epi="bias", place="slice", opts=dict(gemm_kernel=3, gemm_w4=0, gemm_tail=0), tag="no tail"),
    dict(kid=GC.DMA256x256, layout=NN, M=4096, N=3072, K=128, epi="residual", place="tight", opts={}, tag="default, K < 192"),
    dict(kid=GC.W4, layout=NT, M=4096, N=3072, K=4096, epi="plain", place="tight", opts={}, tag="default"),
    dict(kid=GC.DMA64x128, layout=TN, M=200, N=136, K=256, epi="plain", place="tight", opts={}, tag="default small_variant"),
    dict(kid=GC.DMA128, layout=NN, M=2048, N=1024, K=640, epi="bias", place="tight", opts={}, tag="default small_variant"),
    dict(kid=GC.V1, layout=NT, M=2048, N=2688, K=256, epi="plain", place="tight", opts={}, tag="default small_variant"),
    # weight-gradient GEMMs (TN, accumulate into C) on both 256x256 kernels
    dict(kid=GC.DMA256x256, layout=TN, M=4100, N=4100, K=264, epi="accumulate", place="slice", opts=dict(gemm_kernel=3, gemm_w4=0), tag="wgrad"),
    dict(kid=GC.W4, layout=TN, M=4000, N=3304, K=320, epi="accumulate", place="tight", opts=dict(gemm_kernel=3), tag="wgrad"),
]
SKINNY_SHAPES = [(1, 130, 64), (4, 6144, 256), (16, 1000, 200), (7, 72, 1088), (3, 1028, 203), (5, 266, 72), (2, 512, 4104)]
GEMV_SHAPES = [(1, 130, 64), (4, 6144, 256), (16, 1000, 200), (7, 72, 1088), (3, 1028, 128), (5, 266, 72), (2, 512, 4104)]
CASES += _cycle(GC.SKINNY, BASE_EPIS + list(ACT_EPIS), layouts=(NT,), opts=dict(gemv_stream=0), shapes=SKINNY_SHAPES)
CASES += _cycle(GC.GEMV, BASE_EPIS + list(ACT_EPIS), layouts=(NT,), opts={}, shapes=GEMV_SHAPES)
CASES += _cycle(GC.F32, BASE_EPIS, opts={}, shapes=[(64, 64, 256), (100, 124, 200), (130, 66, 203), (257, 200, 130)])


def edge_classes(c):
    """The edge classes a case meets (the coverage matrix of tests/test_gemm_check_cpu.py)."""
    M, N, K = c["M"], c["N"], c["K"]
    out = {LAYOUT_NAME[c["layout"]], "epi:" + c["epi"]}
    out.add("n8" if N % 8 == 0 else ("n4" if N % 4 == 0 else "nodd"))
    out.add("ksmall" if K < 192 else ("k64" if K % 64 == 0 else ("kstep" if K % 8 == 0 else "k8")))
    if c["kid"] in TILE:
        bm, bn = TILE[c["kid"]]
        nwg = -(-M // bm) * -(-N // bn)
        if nwg == 1:
            out.add("grid:single")
        if 0 < nwg % 256 <= 128 and nwg > 1:
            out.add("grid:half")
        if nwg > 256:
            out.add("grid:multi")
    return out


def case_id(c):
    return f"{c['kid']}-{LAYOUT_NAME[c['layout']]}-{c['M']}x{c['N']}x{c['K']}-{c['epi']}-{c['place']}" + (f"-{c['tag']}" if c["tag"] else "")


def _setup(c, seed):
    """Exact-family problem of a case and its stored operands -> (p, A, B, bias, res, dtype, epi)."""
    dtype = torch.float32 if c["kid"] == GC.F32 else torch.bfloat16
    M, N, K = c["M"], c["N"], c["K"]
    p = GC.exact_problem(M, N, K, "cuda", seed)
    A, B = GC.operands(c["layout"], p["A"], p["B"], dtype)
    epi = EPIS[c["epi"]]
    bias = GC.vec_storage(p["bias"], dtype) if epi & GC.EPI_BIAS else None
    res = GC.rows_storage(p["res"], dtype) if epi & GC.EPI_RESIDUAL else None
    return p, A, B, bias, res, dtype, epi


def _want(c, p, epi, dtype):
    """-> ('exact', tensor) or ('bound', (ref, E, c, path))"""
    lin = epi & ~(GC.EPI_GELU_ERF | GC.EPI_QUICK_GELU | GC.EPI_GELU_TANH)
    if c["epi"] in ACT_EPIS:
        pre = GC.exact_reference(p, lin & GC.EPI_BIAS)
        ref, E = GC.act_reference(pre, c["epi"], p["res"] if epi & GC.EPI_RESIDUAL else None)
        return "bound", (ref, E, GC.C["act"], "act")
    ref = GC.exact_reference(p, lin)
    return "exact", (ref.float() if dtype == torch.float32 else GC.rne_bf16(ref))


def _run(c, p, A, B, bias, res, dtype, epi, opts):
    C, guard = GC.out_view(c["M"], c["N"], c["place"], dtype)
    if epi & GC.EPI_ACCUMULATE:
        C.copy_(p["c0"].to(dtype))
    with options(**opts):
        kid = GC.gemm(c["layout"], A, B, c["M"], c["N"], c["K"], C, bias, res, epi, dtype)
    torch.cuda.synchronize()
    guard.verify(f"C ({c['place']})")
    return C, kid


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_gemm_exact(c):
    p, A, B, bias, res, dtype, epi = _setup(c, seed=c["M"] * 7 + c["N"] * 3 + c["K"])
    C, kid = _run(c, p, A, B, bias, res, dtype, epi, c["opts"])
    assert kid == c["kid"], f"launched kernel {kid}, the case is meant for {c['kid']}"
    kind, want = _want(c, p, epi, dtype)
    if kind == "exact":
        GC.check_exact("C", C, want)
    else:
        ref, E, cc, path = want
        GC.check_bound("C", C, ref, E, cc, path)
    if kid in PERSISTENT:
        got = C.clone()
        C0, kid0 = _run(c, p, A, B, bias, res, dtype, epi, dict(c["opts"], gemm_persist=0))
        assert kid0 == kid
        GC.check_exact("C with gemm_persist = 0 vs persistent", C0, got)


# ---- the fused GEMMs --------------------------------------------------------------------------------------------------------
def _call(name, *args):
    from multimeditron_amd._lib import call
    call(name, *args)
    torch.cuda.synchronize()
    return GC.last_kernel()


@pytest.mark.parametrize("kind", ["erf", "quick", "tanh"])
@pytest.mark.parametrize("M,N,K,flags,kid,opts", [
    (300, 136, 72, GC.EPI_BIAS, GC.DMA64x128, {}), (1028, 1024, 1024, GC.EPI_BIAS | GC.EPI_RESIDUAL, GC.DMA64x128, {}),
    (129, 130, 203, GC.EPI_RESIDUAL, GC.DMA64, dict(gemm_kernel=6)), (2048, 1028, 256, GC.EPI_BIAS, GC.DMA128, dict(gemm_kernel=3))])
def test_gemm_act_fwd_keeps_pre(kind, M, N, K, flags, kid, opts):
    """mm_gemm_act_fwd: PRE = bf16(A.B^T + bias) exactly; ACT = act(PRE) (bf16-rounded before the residual add) within the bound."""
    p = GC.exact_problem(M, N, K, "cuda", M + N + K)
    X, W = GC.operands(NT, p["A"], p["B"])
    bias = GC.vec_storage(p["bias"]) if flags & GC.EPI_BIAS else None
    res = GC.rows_storage(p["res"]) if flags & GC.EPI_RESIDUAL else None
    PRE, gp = GC.out_view(M, N, "slice")
    ACT, ga = GC.out_view(M, N, "pad64" if N % 8 else "tight")
    epi = flags | {"erf": GC.EPI_GELU_ERF, "quick": GC.EPI_QUICK_GELU, "tanh": GC.EPI_GELU_TANH}[kind]
    with options(**opts):
        got = _call("mm_gemm_act_fwd", 0, M, N, K, X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), ptr(bias),
                    PRE.data_ptr(), PRE.stride(0), ACT.data_ptr(), ACT.stride(0), ptr(res), res.stride(0) if res is not None else 0,
                    epi, stream())
    assert got == kid
    gp.verify("PRE")
    ga.verify("ACT")
    GC.check_exact("PRE", PRE, GC.rne_bf16(GC.exact_reference(p, flags & GC.EPI_BIAS)))
    ref, E = GC.act_reference(PRE.double(), kind, p["res"] if res is not None else None, round_act=True)
    GC.check_bound("ACT", ACT, ref, E, GC.C["act"], "act")


@pytest.mark.parametrize("M,I,K,opts,kid,kid_bwd", [(512, 256, 256, {}, GC.W4, GC.DMA64x128), (300, 384, 64, {}, GC.DMA256x256, GC.DMA64x128),
                                                     (1000, 1024, 320, dict(gemm_w4=0), GC.DMA256x256, GC.DMA64x128),
                                                     (520, 7168, 256, {}, GC.W4, GC.DMA128),
                                                     (1000, 512, 192, dict(gemm_w4_rowmajor=0), GC.W4, GC.DMA64x128),
                                                     (4096, 3072, 256, {}, GC.W4, GC.W4), (4096, 3072, 256, dict(gemm_w4=0), GC.DMA256x256, GC.DMA256x256)])
def test_gemm_swiglu_fwd_bwd(M, I, K, opts, kid, kid_bwd):
    """mm_gemm_swiglu_fwd: GU = bf16(X.Wgu^T) exactly, ACT = bf16(bf16(silu(gate)) * up) within the bound; mm_gemm_swiglu_bwd:
    dGU from d(act) = bf16(dY.Wd) (exact) and the stored GU.  Both also with gemm_persist = 0, bit-identical."""
    H = 264
    p = GC.exact_problem(M, 2 * I, K, "cuda", M + I)
    X, W = GC.operands(NT, p["A"], p["B"])
    outs = []
    for persist in (1, 0):
        GU, gg = GC.out_view(M, 2 * I, "slice")
        ACT, ga = GC.out_view(M, I, "pad64")
        with options(gemm_persist=persist, **opts):
            got = _call("mm_gemm_swiglu_fwd", 0, M, I, K, X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), GU.data_ptr(),
                        GU.stride(0), ACT.data_ptr(), ACT.stride(0), stream())
        assert got == kid
        gg.verify("GU")
        ga.verify("ACT")
        outs.append((GU.clone(), ACT.clone()))
    GU, ACT = outs[0]
    GC.check_exact("GU", GU, GC.rne_bf16(GC.exact_reference(p)))
    GC.check_exact("GU persist 0", outs[1][0], GU)
    GC.check_exact("ACT persist 0", outs[1][1], ACT)
    ref, E = GC.swiglu_fwd_reference(GU[:, :I].double(), GU[:, I:].double())
    GC.check_bound("ACT", ACT, ref, E, GC.C["swiglu"], "swiglu")
    # backward: dGU [M, 2I] = swiglu'(GU) * (dY [M, H] . Wd [H, I]) -- an NN GEMM with K = H
    q = GC.exact_problem(M, I, H, "cuda", M + I + 1)
    dY, Wd = GC.operands(NN, q["A"], q["B"])
    GUs = GC.rows_storage(GU.double())
    bw = []
    for persist in (1, 0):
        dGU, gd = GC.out_view(M, 2 * I, "tight")
        with options(gemm_persist=persist, **opts):
            got = _call("mm_gemm_swiglu_bwd", 0, M, I, H, dY.data_ptr(), dY.stride(0), Wd.data_ptr(), Wd.stride(0), GUs.data_ptr(),
                        GUs.stride(0), dGU.data_ptr(), dGU.stride(0), stream())
        assert got == kid_bwd
        gd.verify("dGU")
        bw.append(dGU.clone())
    GC.check_exact("dGU persist 0", bw[1], bw[0])
    dact = GC.rne_bf16(GC.exact_reference(q)).double()
    dg, E_dg, du, E_du = GC.swiglu_bwd_reference(GU[:, :I].double(), GU[:, I:].double(), dact)
    GC.check_bound("dgate", bw[0][:, :I], dg, E_dg, GC.C["swiglu"], "swiglu")
    GC.check_bound("dup", bw[0][:, I:], du, E_du, GC.C["swiglu"], "swiglu")


@pytest.mark.parametrize("M,Hq,Hkv,K,bias,opts,kid", [(512, 4, 1, 256, False, {}, GC.W4), (300, 3, 2, 192, True, {}, GC.W4),
                                                      (1000, 8, 2, 130, True, {}, GC.DMA256x256),
                                                      (2049, 28, 4, 320, True, dict(gemm_w4=0), GC.DMA256x256)])
def test_gemm_rope_fwd(M, Hq, Hkv, K, bias, opts, kid):
    """mm_gemm_rope_fwd: the v columns equal bf16(X.W^T + b) bit for bit; the q / k heads are the rotation of that bf16
    output (exact products, then RoPE within the bound); persistent and one-tile-per-workgroup runs bit-identical."""
    D = 128
    N, cols = (Hq + 2 * Hkv) * D, (Hq + Hkv) * D
    p = GC.exact_problem(M, N, K, "cuda", M + N + K)
    X, W = GC.operands(NT, p["A"], p["B"])
    b = GC.vec_storage(p["bias"]) if bias else None
    g = torch.Generator(device="cuda").manual_seed(5)
    ang = torch.rand(M, D // 2, device="cuda", generator=g) * 6.0
    cos, sin = torch.cos(ang).contiguous(), torch.sin(ang).contiguous()
    outs = []
    for persist in (1, 0):
        Q, gq = GC.out_view(M, N, "slice")
        with options(gemm_persist=persist, **opts):
            got = _call("mm_gemm_rope_fwd", 0, M, N, K, X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), ptr(b), Q.data_ptr(),
                        Q.stride(0), cols, D, cos.data_ptr(), sin.data_ptr(), stream())
        assert got == kid
        gq.verify("QKV")
        outs.append(Q.clone())
    GC.check_exact("QKV persist 0", outs[1], outs[0])
    lin = GC.rne_bf16(GC.exact_reference(p, GC.EPI_BIAS if bias else 0))
    GC.check_exact("v columns", outs[0][:, cols:], lin[:, cols:])
    ref, E = GC.rope_reference(lin.double(), cos, sin, cols)
    GC.check_bound("q|k heads", outs[0][:, :cols], ref[:, :cols], E[:, :cols], GC.C["rope"], "rope")


# ---- decode fusions (gemv_stream_kernel) --------------------------------------------------------------------------------------
def _norm_w(K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (1.0 + 0.25 * torch.randn(K, device="cuda", generator=g)).to(torch.bfloat16)


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("M,N,K", [(4, 4104, 1024), (1, 130, 200), (16, 1000, 2048), (3, 266, 72)])
def test_decode_linear(M, N, K, norm):
    p = GC.exact_problem(M, N, K, "cuda", M + N + K)
    X, W = GC.operands(NT, p["A"], p["B"])
    b, res = GC.vec_storage(p["bias"]), GC.rows_storage(p["res"])
    nw = _norm_w(K, 1) if norm else None
    C, gc_ = GC.out_view(M, N, "pad64" if N % 4 else "slice")
    assert _call("mm_decode_linear", 0, M, N, K, X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), b.data_ptr(), res.data_ptr(),
                 res.stride(0), C.data_ptr(), C.stride(0), ptr(nw), 1e-5, stream()) == GC.GEMV
    gc_.verify("C")
    if not norm:
        GC.check_exact("C", C, GC.rne_bf16(GC.exact_reference(p, GC.EPI_BIAS | GC.EPI_RESIDUAL)))
        return
    xn = GC.rmsnorm_x(X, nw, 1e-5)
    ref, E = GC.bound_reference(xn, W, GC.EPI_BIAS | GC.EPI_RESIDUAL, bias=b, res=res)
    GC.check_bound("C", C, ref, E + GC.norm_E(xn, W), GC.C["norm"], "norm")


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("M,I,K", [(4, 1024, 1024), (1, 72, 200), (16, 2368, 512), (7, 260, 1088)])
def test_decode_gateup_swiglu(M, I, K, norm):
    p = GC.exact_problem(M, 2 * I, K, "cuda", M + I + K)
    X, W = GC.operands(NT, p["A"], p["B"])
    nw = _norm_w(K, 2) if norm else None
    ACT, ga = GC.out_view(M, I, "slice")
    assert _call("mm_decode_gateup_swiglu", 0, M, I, K, X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), ACT.data_ptr(),
                 ACT.stride(0), ptr(nw), 1e-5, stream()) == GC.GEMV
    ga.verify("ACT")
    if not norm:
        gu = GC.rne_bf16(GC.exact_reference(p)).double()
        ref, E = GC.swiglu_fwd_reference(gu[:, :I], gu[:, I:])
        GC.check_bound("ACT", ACT, ref, E, GC.C["swiglu"], "swiglu")
        return
    xn = GC.rmsnorm_x(X, nw, 1e-5)
    gu, Egu = GC.bound_reference(xn, W)
    Egu = Egu + GC.norm_E(xn, W)
    s = GC.silu64(gu[:, :I])
    ref = s * gu[:, I:]
    dsilu = 1.5                                    # |silu'| <= 1.1: the gate's error reaches the product through it
    E = ref.abs() + (s * gu[:, I:]).abs() + dsilu * Egu[:, :I] * gu[:, I:].abs() + s.abs() * Egu[:, I:] + \
        GC.FUNC * (gu[:, :I].abs() + s.abs()) * gu[:, I:].abs()
    GC.check_bound("ACT", ACT, ref, E, GC.C["norm"], "norm")


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("M,Hq,Hkv,K,bias", [(4, 8, 2, 1024, False), (1, 4, 1, 200, True), (16, 28, 4, 512, True), (3, 3, 2, 72, False)])
def test_decode_qkv_rope_append(M, Hq, Hkv, K, bias, norm):
    """QKV and the KV-cache rows: the row of this step receives the roped k / v; every other cache row is a guard."""
    D, Smax, pos = 128, 6, 3
    N, cols = (Hq + 2 * Hkv) * D, (Hq + Hkv) * D
    p = GC.exact_problem(M, N, K, "cuda", M + N + K)
    X, W = GC.operands(NT, p["A"], p["B"])
    b = GC.vec_storage(p["bias"]) if bias else None
    nw = _norm_w(K, 3) if norm else None
    g = torch.Generator(device="cuda").manual_seed(7)
    ang = torch.rand(M, D // 2, device="cuda", generator=g) * 6.0
    cos, sin = torch.cos(ang).contiguous(), torch.sin(ang).contiguous()
    Q, gq = GC.out_view(M, N, "slice")
    gk, gv = (GC.Guarded(M * Smax * Hkv * D, torch.bfloat16, "cuda") for _ in range(2))
    kc = gk.buf[gk.pad:gk.pad + M * Smax * Hkv * D].view(M, Smax, Hkv, D)
    vc = gv.buf[gv.pad:gv.pad + M * Smax * Hkv * D].view(M, Smax, Hkv, D)
    krow, vrow = (gg.view((M, Hkv * D), (Smax * Hkv * D, 1), pos * Hkv * D) for gg in (gk, gv))
    assert _call("mm_decode_qkv_rope_append", 0, M, Hq, Hkv, D, K, X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), ptr(b),
                 Q.data_ptr(), Q.stride(0), cos.data_ptr(), sin.data_ptr(), kc[:, pos].data_ptr(), vc[:, pos].data_ptr(),
                 kc.stride(0), ptr(nw), 1e-6, stream()) == GC.GEMV
    gq.verify("QKV")
    gk.verify("k cache")
    gv.verify("v cache")
    GC.check_exact("k cache row = roped k", krow, Q[:, Hq * D:cols])
    GC.check_exact("v cache row = v", vrow, Q[:, cols:])
    if not norm:
        lin = GC.rne_bf16(GC.exact_reference(p, GC.EPI_BIAS if bias else 0))
        GC.check_exact("v columns", Q[:, cols:], lin[:, cols:])
        ref, E = GC.rope_reference(lin.double(), cos, sin, cols)
        GC.check_bound("q|k heads", Q[:, :cols], ref[:, :cols], E[:, :cols], GC.C["rope"], "rope")
        return
    xn = GC.rmsnorm_x(X, nw, 1e-6)
    lin, El = GC.bound_reference(xn, W, GC.EPI_BIAS if bias else 0, bias=b)
    El = El + GC.norm_E(xn, W)
    ref, E = GC.rope_reference(lin, cos, sin, cols)
    Eh = El[:, :cols].reshape(M, -1, D)                                    # the product's error through the rotation (|cos|, |sin| <= 1)
    Et = E.clone()
    Et[:, :cols] += (Eh + torch.cat([Eh[..., D // 2:], Eh[..., :D // 2]], -1)).reshape(M, cols)
    Et[:, cols:] = El[:, cols:]
    GC.check_bound("QKV", Q, ref, Et, GC.C["norm"], "norm")


# ---- colsum ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("M,N,acc", [(1028, 1024, False), (300, 130, True), (4096, 4100, False), (7, 3, True)])
def test_colsum_exact(dtype, M, N, acc):
    """mm_colsum of exact-family data: out = RNE(fp64 column sum (+ out)) for bf16, the fp64 sum itself for fp32."""
    p = GC.exact_problem(M, N, 8, "cuda", M + N, span=2)
    X = GC.rows_storage(p["res"], dtype, ld=GC.pad8(N) + 8)
    g = GC.Guarded(N, dtype, "cuda")
    out = g.view((N,), (1,), 0)
    base = torch.zeros(N, dtype=torch.float64, device="cuda")
    if acc:
        base = p["c0"][0] * 2.0 ** 6
        out.copy_(base.to(dtype))
    _call("mm_colsum", dt(dtype), X.data_ptr(), M, N, X.stride(0), out.data_ptr(), int(acc), stream())
    g.verify("colsum out")
    ref = p["res"].sum(0) + base
    assert float(((p["res"].abs().sum(0) + base.abs()) / (p["q"].min(0).values)).max()) < 2 ** 24
    GC.check_exact("colsum", out, ref.float() if dtype == torch.float32 else GC.rne_bf16(ref))


# ---- the step's shapes at reduced M, on the default dispatch ---------------------------------------------------------------------
REAL = [  # (name, layout, M, N, K, epi, kernel id)
    ("llama qkv", NT, 512, 6144, 4096, "plain", GC.DMA128),
    ("llama gate|up", NT, 1024, 28672, 4096, "plain", GC.W4),
    ("llama down dgrad", NN, 1024, 14336, 4096, "plain", GC.W4),
    ("llama down wgrad", TN, 4096, 14336, 512, "accumulate", GC.W4),
    ("llama lm_head fwd", NT, 512, 128258, 4096, "plain", GC.W4),
    ("llama lm_head dgrad", NN, 512, 4096, 128258, "plain", GC.DMA128),
    ("llama lm_head wgrad", TN, 128258, 4096, 256, "plain", GC.W4),
    ("qwen2 qkv", NT, 512, 4608, 3584, "bias", GC.DMA128),
    ("qwen2 gate|up", NT, 512, 37888, 3584, "plain", GC.W4),
    ("qwen2 down dgrad", NN, 512, 3584, 18944, "residual", GC.DMA128),
    ("vit patch", NT, 1028, 1024, 588, "bias", GC.DMA64x128),
    ("vit fc1 wgrad", TN, 4096, 1024, 1028, "accumulate", GC.DMA128),
]


@pytest.mark.parametrize("name,layout,M,N,K,epi,kid", REAL, ids=[r[0] for r in REAL])
def test_real_shapes(name, layout, M, N, K, epi, kid):
    """Llama-3.1-8B (H 4096, I 14336, qkv 6144, V 128 258), Qwen2-7B (3584 / 18944, 28/4 heads, qkv bias) and ViT-L/14 (1024 /
    4096, patch K 588 in a 640-wide row) at reduced M, default dispatch: exact, kernel id asserted; logits at the padded ldc."""
    c = dict(kid=kid, layout=layout, M=M, N=N, K=K, epi=epi, place="pad64" if N % 8 else "tight", opts={}, tag=name)
    ld = 640 if name == "vit patch" else None
    p = GC.exact_problem(M, N, K, "cuda", M + N + K, span=1 if K > 65536 else 3, amp=4 if K > 65536 else 8)
    A, B = GC.operands(layout, p["A"], p["B"], lda=ld, ldb=ld)
    e = EPIS[epi]
    bias = GC.vec_storage(p["bias"]) if e & GC.EPI_BIAS else None
    res = GC.rows_storage(p["res"]) if e & GC.EPI_RESIDUAL else None
    C, got = _run(c, p, A, B, bias, res, torch.bfloat16, e, {})
    assert got == kid, f"{name}: launched kernel {got}, expected {kid}"
    GC.check_exact(name, C, GC.rne_bf16(GC.exact_reference(p, e)))


# ---- 32-bit offset thresholds -------------------------------------------------------------------------------------------------
THRESH = [  # (what, layout, M, N, K, lda, ldb, kernel id): just below the limit (fast path) and at it (fallback)
    ("TN K*lda*2 below 4 GiB", TN, 256, 256, 32768, 65528, 264, GC.DMA64x128),
    ("TN K*lda*2 at 4 GiB", TN, 256, 256, 32768, 65536, 264, GC.V1),
    ("NN K*ldb*2 below 4 GiB", NN, 256, 256, 32768, 32776, 65528, GC.DMA64x128),
    ("NN K*ldb*2 at 4 GiB", NN, 256, 256, 32768, 32776, 65536, GC.V1),
    ("gemv N*ldb*2 below 4 GiB", NT, 4, 65536, 64, 72, 32760, GC.GEMV),
    ("gemv N*ldb*2 at 4 GiB", NT, 4, 65536, 64, 72, 32768, GC.SKINNY),
]


@pytest.mark.parametrize("what,layout,M,N,K,lda,ldb,kid", THRESH, ids=[t[0] for t in THRESH])
def test_offset_thresholds(what, layout, M, N, K, lda, ldb, kid):
    """The dispatcher's 32-bit offset limits on both sides, exact-family data, the fp64 reference in K-chunks."""
    rows_b = K if layout != NT else N
    need = 2 * ((K + 72) * lda if layout == TN else (M + 8) * lda) + 2 * (rows_b + 72) * ldb
    free, _ = torch.cuda.mem_get_info()
    if free < need * 1.25 + (1 << 30):
        pytest.skip(f"needs {need / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB free")
    p = GC.exact_problem(M, N, K, "cuda", K + lda + ldb)
    A, B = GC.operands(layout, p["A"], p["B"], lda=lda, ldb=ldb)
    del p["A"], p["B"]
    c = dict(kid=kid, layout=layout, M=M, N=N, K=K, epi="plain", place="tight", opts={}, tag=what)
    C, got = _run(c, p, A, B, None, None, torch.bfloat16, 0, {})
    assert got == kid, f"{what}: launched kernel {got}, expected {kid}"
    a_of = (lambda k0, k1: A[k0:k1].t()) if layout == TN else (lambda k0, k1: A[:, k0:k1])
    b_of = (lambda k0, k1: B[:, k0:k1]) if layout == NT else (lambda k0, k1: B[k0:k1].t())
    ref = GC.exact_reference_chunked(a_of, b_of, M, N, K, p["q"])
    GC.check_exact(what, C, GC.rne_bf16(ref))
    del A, B
    torch.cuda.empty_cache()
