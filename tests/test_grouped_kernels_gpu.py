"""The grouped launches (include/mm_hip.h, "grouped launches": the expert as a batch dimension) against the stand-alone entry points,
problem by problem and BIT FOR BIT: a grouped launch is the stand-alone kernel's arithmetic on every problem, so there is no
tolerance anywhere in this file.  Outputs sit inside guard rows and columns of a fixed pattern that must survive."""
import ctypes
from contextlib import contextmanager

import pytest
import torch

pytestmark = pytest.mark.gpu

BIAS, QUICK_GELU, RESIDUAL, ACCUMULATE = 1, 4, 8, 16
NT, NN, TN = 0, 1, 2
SHAPES = [(68, 128, 128), (130, 136, 72), (257, 384, 264)]      # the last: past the 128 / 256 tile edges, several K-steps, a ragged last one
CASES = [(NT, 0), (NT, BIAS), (NT, BIAS | QUICK_GELU), (NT, BIAS | RESIDUAL), (NN, 0), (NN, BIAS), (TN, 0), (TN, BIAS), (TN, ACCUMULATE)]
GROUPS = [1, 3, 16]
GUARD = 8                                                       # guard columns behind N (ldc stays a multiple of 8); one guard row above and below


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@contextmanager
def _recorded():
    """names of the library calls made through multimeditron_amd.kernels inside the block"""
    from multimeditron_amd import kernels
    names, real = [], kernels.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)

    kernels.call = spy
    try:
        yield names
    finally:
        kernels.call = real


def pad8(n):
    return (n + 7) // 8 * 8


def _pattern(rows, cols, dtype):
    """the fixed guard pattern (also C's starting value under ACCUMULATE): small integers, exact in bf16"""
    i = torch.arange(rows * cols, device="cuda", dtype=torch.float32).view(rows, cols)
    return ((i * 7) % 13 - 6).to(dtype)


def _guarded(M, N, dtype):
    """-> (buffer [M + 2, ld], its view [M, N] inside the guards)"""
    buf = _pattern(M + 2, pad8(N) + GUARD, dtype)
    return buf, buf[1:M + 1, :N]


def _guards_intact(buf, M, N):
    ref = _pattern(buf.shape[0], buf.shape[1], buf.dtype)
    return torch.equal(buf[0], ref[0]) and torch.equal(buf[M + 1], ref[M + 1]) and torch.equal(buf[:, N:], ref[:, N:])


def _mat(rows, cols, dtype, gen, pool=None):
    """[rows, cols] with the row stride padded to a multiple of 8 and zeros in the padding; from `pool` (a carving function) when given"""
    ld = pad8(cols)
    t = pool(rows * ld).view(rows, ld) if pool is not None else torch.zeros((rows, ld), dtype=dtype, device="cuda")
    t.zero_()
    t[:, :cols] = (torch.randn((rows, cols), generator=gen) * 0.5).to(dtype).cuda()
    return t[:, :cols]


def _problems(dtype, layout, M, N, K, g, epi, gen, same_a=False, uneven=False):
    pool = None
    if uneven:                          # every operand inside ONE allocation, at spacings that differ from problem to problem
        big = torch.zeros(g * 4 * (max(M, K) + 8) * (pad8(max(M, N, K)) + 8) + 4096, dtype=dtype, device="cuda")
        state = {"off": 0, "i": 0}

        def pool(n):
            state["off"] += 8 * (1 + (state["i"] * 5) % 7)       # gaps of 8 .. 56 elements: 16-byte aligned, never the same twice in a row
            state["i"] += 1
            t = big[state["off"]:state["off"] + n]
            state["off"] += pad8(n)
            return t

    a_shape = (K, M) if layout == TN else (M, K)
    b_shape = (N, K) if layout == NT else (K, N)
    a0 = _mat(*a_shape, dtype, gen, pool)
    As = [a0 if same_a else (a0 if p == 0 else _mat(*a_shape, dtype, gen, pool)) for p in range(g)]
    Bs = [_mat(*b_shape, dtype, gen, pool) for _ in range(g)]
    biases = [(torch.randn(N, generator=gen) * 0.5).to(dtype).cuda() for _ in range(g)] if epi & BIAS else None
    res = [_mat(M, N, dtype, gen, pool) for _ in range(g)] if epi & RESIDUAL else None
    return As, Bs, biases, res


def _check_gemm(dtype, layout, M, N, K, g, epi, gen, **kw):
    from multimeditron_amd import kernels as Kn
    As, Bs, biases, res = _problems(dtype, layout, M, N, K, g, epi, gen, **kw)
    act, acc = epi & QUICK_GELU, bool(epi & ACCUMULATE)
    got = [_guarded(M, N, dtype) for _ in range(g)]
    with _recorded() as names:
        Kn.gemm_batched(layout, As, Bs, M, N, K, [c for _, c in got], biases=biases, residuals=res, act=act, accumulate=acc)
    assert names == ["mm_gemm_batched"], names                 # one grouped launch, not the wrapper's per-problem loop
    torch.cuda.synchronize()
    for p in range(g):
        buf, c = _guarded(M, N, dtype)
        Kn.gemm(layout, As[p], Bs[p], M, N, K, out=c, bias=biases[p] if biases else None, residual=res[p] if res else None, act=act,
                accumulate=acc)
        assert torch.equal(got[p][1], c), (p, float((got[p][1].float() - c.float()).abs().max()))
        assert _guards_intact(got[p][0], M, N) and _guards_intact(buf, M, N), p
    if g > 1 and not kw.get("same_a"):
        assert not torch.equal(got[0][1], got[1][1])           # the problems really differ


@pytest.mark.parametrize("layout,epi", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_gemm_batched_equals_gemm(dtype, shape, layout, epi):
    gen = torch.Generator().manual_seed(11)
    for g in GROUPS:
        _check_gemm(dtype, layout, *shape, g, epi, gen)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("mode", ["same_a", "uneven"])
def test_gemm_batched_shared_and_unevenly_spaced_operands(dtype, mode):
    """the patch embedding's GEMM reads the same patches for every expert; operands need not be evenly spaced"""
    gen = torch.Generator().manual_seed(12)
    for layout, epi in ((NT, BIAS | RESIDUAL), (TN, ACCUMULATE), (NN, 0)):
        _check_gemm(dtype, layout, 257, 384, 264, 3, epi, gen, **{mode: True})


@pytest.mark.parametrize("epi", [BIAS | QUICK_GELU, BIAS | QUICK_GELU | RESIDUAL, QUICK_GELU], ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_act_fwd_batched_equals_gemm_act_fwd(shape, epi):
    from multimeditron_amd import kernels as Kn
    from multimeditron_amd._lib import MM_BF16, call
    M, N, K = shape
    dtype = torch.bfloat16
    gen = torch.Generator().manual_seed(13)
    st = torch.cuda.current_stream().cuda_stream
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts]) if ts is not None else None
    for g in GROUPS:
        Xs, Ws, biases, res = _problems(dtype, NT, M, N, K, g, epi, gen)
        pre = [_guarded(M, N, dtype) for _ in range(g)]
        act = [_guarded(M, N, dtype) for _ in range(g)]
        call("mm_gemm_act_fwd_batched", MM_BF16, g, M, N, K, arr(Xs), Xs[0].stride(0), arr(Ws), Ws[0].stride(0), arr(biases),
             arr([c for _, c in pre]), pre[0][1].stride(0), arr([c for _, c in act]), act[0][1].stride(0), arr(res),
             res[0].stride(0) if res else 0, epi, st)
        torch.cuda.synchronize()
        for p in range(g):
            rp, ra = _guarded(M, N, dtype), _guarded(M, N, dtype)
            call("mm_gemm_act_fwd", MM_BF16, M, N, K, Xs[p].data_ptr(), Xs[p].stride(0), Ws[p].data_ptr(), Ws[p].stride(0),
                 biases[p].data_ptr() if biases else None, rp[1].data_ptr(), rp[1].stride(0), ra[1].data_ptr(), ra[1].stride(0),
                 res[p].data_ptr() if res else None, res[p].stride(0) if res else 0, epi, st)
            assert torch.equal(pre[p][1], rp[1]) and torch.equal(act[p][1], ra[1]), p
            assert _guards_intact(pre[p][0], M, N) and _guards_intact(act[p][0], M, N), p
        # the tensor-level wrapper: one grouped launch, the same bits
        x = torch.cat([t.contiguous() for t in Xs]) if K % 8 == 0 else None
        if x is not None and g > 1:
            with _recorded() as names:
                out = Kn.linear_act_fwd_batched(x, [w for w in Ws], biases, epi & QUICK_GELU,
                                                torch.cat([r.contiguous() for r in res]) if res else None)
            assert names == ["mm_gemm_act_fwd_batched"]
            for p in range(g):
                assert torch.equal(out[0][p * M:(p + 1) * M], pre[p][1]) and torch.equal(out[1][p * M:(p + 1) * M], act[p][1])


def test_gemm_batched_refuses_what_fills_the_chip_alone():
    """M = N = K = 4096 takes the 4-wave 256x256 kernel in mm_gemm: the grouped entry point returns MM_ERR_UNSUPPORTED before any
    launch (nothing is written) and the tensor-level wrapper loops mm_gemm: the same bits."""
    from multimeditron_amd import _lib, kernels as Kn
    M = N = K = 4096
    gen = torch.Generator().manual_seed(14)
    a = (torch.randn((M, K), generator=gen) * 0.1).to(torch.bfloat16).cuda()
    Bs = [(torch.randn((N, K), generator=gen) * 0.1).to(torch.bfloat16).cuda() for _ in range(2)]
    Cs = [torch.full((M, N), 3.0, dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    rc = _lib.lib().mm_gemm_batched(_lib.MM_BF16, NT, 2, M, N, K, arr([a, a]), K, arr(Bs), K, arr(Cs), N, None, None, 0, 0,
                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _lib.ERR_UNSUPPORTED
    assert all(bool((c == 3.0).all()) for c in Cs)
    with _recorded() as names:
        Kn.gemm_batched(NT, [a, a], Bs, M, N, K, Cs)
    assert names == ["mm_gemm_batched", "mm_gemm", "mm_gemm"]
    for p in range(2):
        assert torch.equal(Cs[p], Kn.gemm(NT, a, Bs[p], M, N, K))


# ---------------------------------------------------------------------------------------------- LayerNorm, reduce, column sums
E = 3


def _rows_per_block():
    from multimeditron_amd import kernels as Kn
    r = 1
    while Kn.norm_bwd_blocks(r + 1) == 1:
        r += 1
    return r


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("with_dres", [False, True], ids=["no-dres", "dres"])
@pytest.mark.parametrize("H", [128, 1032])
@pytest.mark.parametrize("R", [1, 68, "block+1"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_layernorm_batched_equals_stand_alone(dtype, R, H, with_dres, accumulate):
    from multimeditron_amd import kernels as Kn
    if R == "block+1":
        R = _rows_per_block() + 1                # the backward's second workgroup of an expert holds one row
    gen = torch.Generator().manual_seed(15)
    rnd = lambda *s: (torch.randn(s, generator=gen)).to(dtype).cuda()
    x, dy = rnd(E * R, H), rnd(E * R, H)
    dres = rnd(E * R, H) if with_dres else None
    ws, bs = [rnd(H) + 1 for _ in range(E)], [rnd(H) for _ in range(E)]
    old_w, old_b = [rnd(H) for _ in range(E)], [rnd(H) for _ in range(E)]      # what the gradients hold before (read only when accumulating)
    y, mean, rstd = Kn.layernorm_fwd_batched(x, ws, bs, 1e-5)
    dx, dwp, dbp = Kn.layernorm_bwd_batched(dy, x, ws, mean, rstd, dres)
    nb = Kn.norm_bwd_blocks(R)
    assert dwp.shape == (E * nb, H) and dbp.shape == (E * nb, H)
    gw, gb = [t.clone() for t in old_w], [t.clone() for t in old_b]
    Kn.reduce_partials2_batched(dwp, dbp, gw, gb, accumulate, accumulate)
    torch.cuda.synchronize()
    for e in range(E):
        sl = slice(e * R, (e + 1) * R)
        y1, m1, r1 = Kn.layernorm_fwd(x[sl], ws[e], bs[e], 1e-5)
        assert torch.equal(y[sl], y1) and torch.equal(mean[sl], m1) and torch.equal(rstd[sl], r1), e
        dx1, dwp1, dbp1 = Kn.layernorm_bwd(dy[sl], x[sl], ws[e], m1, r1, dres[sl] if with_dres else None)
        assert torch.equal(dx[sl], dx1), e
        assert torch.equal(dwp[e * nb:(e + 1) * nb], dwp1) and torch.equal(dbp[e * nb:(e + 1) * nb], dbp1), e      # an expert owns its blocks
        gw1, gb1 = old_w[e].clone(), old_b[e].clone()
        Kn.reduce_partials2(dwp1, dbp1, gw1, gb1, accumulate, accumulate)
        assert torch.equal(gw[e], gw1) and torch.equal(gb[e], gb1), e
    if R > 1:
        assert not torch.equal(gw[0], gw[1])


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("N", [128, 1032])
@pytest.mark.parametrize("R", [1, 68, 257])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_colsum_batched_equals_colsum(dtype, R, N, accumulate):
    from multimeditron_amd import kernels as Kn
    gen = torch.Generator().manual_seed(16)
    x = torch.randn((E * R, N), generator=gen).to(dtype).cuda()
    old = [torch.randn(N, generator=gen).to(dtype).cuda() for _ in range(E)]
    got = [t.clone() for t in old]
    Kn.colsum_batched(x, got, accumulate)
    torch.cuda.synchronize()
    for e in range(E):
        ref = old[e].clone()
        Kn.colsum(x[e * R:(e + 1) * R], ref, accumulate)
        assert torch.equal(got[e], ref), e
    assert not torch.equal(got[0], got[1])
