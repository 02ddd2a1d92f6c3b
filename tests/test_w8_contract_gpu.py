"""The MXFP8 weight-only kernels held to EXACT results.

1. The quantiser: dequant(quant(W)) on the device equals tests/w8_check.py's dequant_ref(quant_ref(W)) bit for bit, on matrices that
   meet every branch of the format (zero blocks, negative zeros, magnitudes over 2^+-20 and more, both sides of the 448 boundary,
   e4m3 subnormals), read through a row stride with NaN in the padding, the packed buffer in a guarded storage of exactly
   mm_mxfp8_bytes and W' in a guarded storage of its own.  The buffer's layout is the library's business: no test looks inside.

2. The decode kernels: an e4m3 value times a power of two is a bf16 number, so the dequantised matrix W' is an ordinary bf16
   tensor and every mm_decode_*_w8 call must return THE BITS of the bf16 entry point run on W' -- which tests/test_gemm_contract_gpu.py
   holds to exact and fp64 bounds.  No tolerance.  Both calls must report the streaming kernel (22 and 21): against the skinny kernel
   the comparison would not mean what it says."""
import pytest
import torch

from multimeditron_amd import kernels as K
from multimeditron_amd._lib import call
from tests import gemm_check as GC
from tests import kernel_check as KC
from tests import w8_check as W8
from tests.kernel_check import options, ptr, stream

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
GEMV_W8 = 22


def _call(name, *args):
    call(name, *args)
    torch.cuda.synchronize()
    return GC.last_kernel()


def _packed_guard(N, Kd):
    """A guarded storage of exactly mm_mxfp8_bytes(N, K) bytes (as bf16 elements: the size is a multiple of 16)."""
    nbytes = K.mxfp8_bytes(N, Kd)
    assert nbytes % 16 == 0
    g = KC.Guarded(nbytes // 2, BF, "cuda")
    return g.view((nbytes // 2,), (1,)), g


def _quant(W):
    """W (a strided bf16 view) -> (packed view, its guard); every byte of the buffer must have been written, none outside it."""
    N, Kd = W.shape
    pk, g = _packed_guard(N, Kd)
    call("mm_quant_mxfp8", W.data_ptr(), W.stride(0), N, Kd, pk.data_ptr(), stream())
    torch.cuda.synchronize()
    g.verify("packed")
    return pk, g


# ---- 1. the quantiser ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K_", [32, 256, 4128])
@pytest.mark.parametrize("N", [1, 17, 1003])
def test_quantiser_matches_the_reference_bitwise(N, K_):
    w = W8.sample_matrix(N, K_, seed=N * 7 + K_)
    want = W8.roundtrip_ref(w)
    W = GC.kc_storage(w.cuda())                               # row stride K + 16, NaN in the padding and in the rows past N
    assert W.stride(0) > K_ and bool(torch.isnan(W.as_strided((N, W.stride(0) - K_), (W.stride(0), 1), W.storage_offset() + K_)).all())
    pk, g = _quant(W)
    Wd, gd = GC.out_view(N, K_, "slice")
    call("mm_dequant_mxfp8", pk.data_ptr(), N, K_, Wd.data_ptr(), Wd.stride(0), stream())
    torch.cuda.synchronize()
    gd.verify("Wd")
    g.verify("packed after dequant")
    KC.check_bits("dequant(quant(W)) vs the reference", Wd, want)
    # the python wrappers: the same bytes, the same matrix; and a second quantisation of W' changes nothing
    pk2 = K.quant_mxfp8(W)
    assert torch.equal(pk2, pk.view(torch.uint8))
    wd2 = K.dequant_mxfp8(K.quant_mxfp8(Wd), N, K_)
    KC.check_bits("requantised W'", wd2, want)


# ---- 2. the kernels ------------------------------------------------------------------------------------------------------------
def _randn(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, device="cuda", generator=g) * scale + shift).to(BF)


def _weights(N, Kd, seed):
    """-> (packed view, W' stored with NaN padding): random weights at the decode-chain test's scale, whose blocks also carry the
    format's edge cases when seed is odd."""
    w = _randn((N, Kd), seed, 0.05)
    if seed & 1:
        w[::5] = W8.sample_matrix(len(range(0, N, 5)), Kd, seed).cuda().clamp(-4, 4)
    pk, _ = _quant(GC.kc_storage(w))
    wd = K.dequant_mxfp8(pk, N, Kd)
    assert not bool(torch.equal(wd, w))                       # the quantisation does round: W' is another matrix
    return pk, GC.kc_storage(wd)


def _norm_w(Kd, seed):
    return _randn((Kd,), seed, 0.3, 1.0)


LINEAR = (
    # the epilogues, N = 1003 at a padded ldc (a tail inside a 16-row block), K = 256 (one partial ring round)
    [(3, 1003, 256, b, r, n) for b in (False, True) for r in (False, True) for n in (False, True)]
    + [(M, 1003, 256, True, True, n) for M in (1, 16) for n in (False, True)]
    # a workgroup walks more than one row block, the last block partial
    + [(3, 16424, 256, True, True, False), (16, 16424, 256, False, True, True)]
    # more than one ring round, ending mid-round (257 K-steps: 33 per wave)
    + [(3, 1003, 8224, True, False, False), (3, 40, 8224, False, True, False)]
    # waves with no K-steps (5 K-steps for 8 waves)
    + [(16, 1003, 160, True, True, True), (1, 1003, 160, False, False, False), (3, 1003, 160, True, False, True)]
    # a single K-step, a single row
    + [(3, 1, 32, False, False, False), (16, 17, 4128, True, True, True)])


def _linear(M, N, Kd, bias, res, norm, seed=0):
    pk, Wd = _weights(N, Kd, M + N + Kd + seed)
    X = GC.kc_storage(_randn((M, Kd), 11 + seed))
    b = GC.vec_storage(_randn((N,), 12, 0.3)) if bias else None
    R = GC.rows_storage(_randn((M, N), 13)) if res else None
    nw = _norm_w(Kd, 14) if norm else None
    ldr = R.stride(0) if res else 0
    C8, g8 = GC.out_view(M, N, "pad64")
    C16, g16 = GC.out_view(M, N, "pad64")
    run8 = lambda: _call("mm_decode_linear_w8", 0, M, N, Kd, X.data_ptr(), X.stride(0), pk.data_ptr(), ptr(b), ptr(R), ldr, C8.data_ptr(),
                         C8.stride(0), ptr(nw), 1e-5, stream())
    run16 = lambda: _call("mm_decode_linear", 0, M, N, Kd, X.data_ptr(), X.stride(0), Wd.data_ptr(), Wd.stride(0), ptr(b), ptr(R), ldr,
                          C16.data_ptr(), C16.stride(0), ptr(nw), 1e-5, stream())
    return run8, run16, [("C", C8, C16)], [("C w8", g8), ("C bf16", g16)]


def _gateup(M, I, Kd, norm, seed=0):
    pk, Wd = _weights(2 * I, Kd, M + I + Kd + seed)
    X = GC.kc_storage(_randn((M, Kd), 21 + seed))
    nw = _norm_w(Kd, 22) if norm else None
    A8, g8 = GC.out_view(M, I, "slice")
    A16, g16 = GC.out_view(M, I, "slice")
    run8 = lambda: _call("mm_decode_gateup_swiglu_w8", 0, M, I, Kd, X.data_ptr(), X.stride(0), pk.data_ptr(), A8.data_ptr(), A8.stride(0),
                         ptr(nw), 1e-5, stream())
    run16 = lambda: _call("mm_decode_gateup_swiglu", 0, M, I, Kd, X.data_ptr(), X.stride(0), Wd.data_ptr(), Wd.stride(0), A16.data_ptr(),
                          A16.stride(0), ptr(nw), 1e-5, stream())
    return run8, run16, [("ACT", A8, A16)], [("ACT w8", g8), ("ACT bf16", g16)]


def _qkv(M, Hq, Hkv, Kd, bias, norm, seed=0):
    D, Smax, pos = 128, 6, 3
    N = (Hq + 2 * Hkv) * D
    pk, Wd = _weights(N, Kd, M + N + Kd + seed)
    X = GC.kc_storage(_randn((M, Kd), 31 + seed))
    b = GC.vec_storage(_randn((N,), 32, 0.3)) if bias else None
    nw = _norm_w(Kd, 33) if norm else None
    g = torch.Generator(device="cuda").manual_seed(7)
    ang = torch.rand(M, D // 2, device="cuda", generator=g) * 6.0
    cos, sin = torch.cos(ang).contiguous(), torch.sin(ang).contiguous()
    outs, guards, runs = [], [], []
    for tag, name, wargs in (("w8", "mm_decode_qkv_rope_append_w8", (pk.data_ptr(),)),
                             ("bf16", "mm_decode_qkv_rope_append", (Wd.data_ptr(), Wd.stride(0)))):
        Q, gq = GC.out_view(M, N, "slice")
        gk, gv = (KC.Guarded(M * Smax * Hkv * D, BF, "cuda") for _ in range(2))
        krow, vrow = (gg.view((M, Hkv * D), (Smax * Hkv * D, 1), pos * Hkv * D) for gg in (gk, gv))   # every other cache row is a guard
        runs.append(lambda name=name, wargs=wargs, Q=Q, krow=krow, vrow=vrow: _call(
            name, 0, M, Hq, Hkv, D, Kd, X.data_ptr(), X.stride(0), *wargs, ptr(b), Q.data_ptr(), Q.stride(0), cos.data_ptr(), sin.data_ptr(),
            krow.data_ptr(), vrow.data_ptr(), Smax * Hkv * D, ptr(nw), 1e-6, stream()))
        outs.append((Q, krow, vrow))
        guards += [(f"QKV {tag}", gq), (f"k cache {tag}", gk), (f"v cache {tag}", gv)]
    pairs = [(n, a, b_) for n, a, b_ in zip(("QKV", "k cache row", "v cache row"), outs[0], outs[1])]
    return runs[0], runs[1], pairs, guards


def _check(case):
    run8, run16, pairs, guards = case
    assert run8() == GEMV_W8
    assert run16() == GC.GEMV
    KC.verify_guards(guards)
    for name, got, want in pairs:
        assert bool(torch.isfinite(want.float()).all())
        KC.check_bits(f"{name}: MXFP8 kernel vs the bf16 kernel on W'", got, want)


@pytest.mark.parametrize("M,N,K_,bias,res,norm", LINEAR)
def test_decode_linear_w8(M, N, K_, bias, res, norm):
    _check(_linear(M, N, K_, bias, res, norm))


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("K_", [256, 1024])
@pytest.mark.parametrize("I", [576, 580])
@pytest.mark.parametrize("M", [1, 3, 16])
def test_decode_gateup_swiglu_w8(M, I, K_, norm):
    _check(_gateup(M, I, K_, norm))


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("K_", [256, 1024])
@pytest.mark.parametrize("Hq,Hkv", [(4, 1), (4, 2)])
@pytest.mark.parametrize("M", [1, 3, 16])
def test_decode_qkv_rope_append_w8(M, Hq, Hkv, K_, bias, norm):
    _check(_qkv(M, Hq, Hkv, K_, bias, norm))


@pytest.mark.parametrize("mode", ["linear", "gateup", "qkv"])
def test_the_other_cache_policy_gives_the_same_bits(mode):
    """gemv_nt flipped (the non-temporal policy on the W loads is another instantiation of the kernel): same bits, same ids."""
    make = {"linear": lambda: _linear(3, 1003, 1056, True, True, True, seed=1), "gateup": lambda: _gateup(3, 580, 1056, True, seed=1),
            "qkv": lambda: _qkv(3, 4, 2, 1056, True, True, seed=1)}[mode]
    first = make()
    _check(first)
    with options(gemv_nt=0 if KC.get_option("gemv_nt") else 1):
        second = make()
        _check(second)
    for (name, a, _), (_, b, _) in zip(first[2], second[2]):
        KC.check_bits(f"{name}: gemv_nt flipped", b, a)


def test_refusals_on_the_device():
    """K % 32 and an x that does not fit the stage: MM_ERR_UNSUPPORTED, nothing launched (the last kernel id stays)."""
    X = torch.zeros(16, 8192, dtype=BF, device="cuda")
    pk = torch.zeros(K.mxfp8_bytes(16, 8192), dtype=torch.uint8, device="cuda")
    C = torch.zeros(16, 64, dtype=BF, device="cuda")
    _check(_linear(1, 17, 32, False, False, False))
    before = GC.last_kernel()
    assert KC.rc("mm_decode_linear_w8", 0, 16, 16, 8192, X.data_ptr(), 8192, pk.data_ptr(), None, None, 0, C.data_ptr(), 64, None, 0.0) == -3
    assert KC.rc("mm_decode_linear_w8", 0, 4, 16, 48, X.data_ptr(), 48, pk.data_ptr(), None, None, 0, C.data_ptr(), 64, None, 0.0) == -3
    assert GC.last_kernel() == before
    assert not bool(C.any())
