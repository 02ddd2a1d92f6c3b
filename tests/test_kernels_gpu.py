"""Kernel-level parity (GPU): every libmmhip entry point, called through the C ABI (ctypes), against a plain
PyTorch fp32 computation of the same op on the same seeded inputs.

Tolerances: MM_F32 kernels 2e-5 rel-L2 (exact-fp32 MFMA / VALU, different summation order);
MM_BF16 kernels 1e-2 rel-L2 vs the fp32 result computed from the SAME bf16-rounded inputs (bf16 output rounding
is 2^-9 relative per element; typical measured values are 2e-3..4e-3)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import embed_check as EC
from tests import gemm_check as GC
from tests import optim_check as OC
from tests import rowwise_check as RC
from tests.kernel_check import check_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from multimeditron_amd import kernels
    return kernels


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * scale
    return x.to(dtype)


TOL = {torch.float32: 2e-5, torch.bfloat16: 1e-2}


def test_lane_maps(K):
    """Pins the hardware lane maps every MFMA kernel here assumes (exact small-integer data)."""
    from multimeditron_amd._lib import call
    g = torch.Generator().manual_seed(0)
    # --- MFMA 32x32x16: A[i][k]: lane l holds A[l&31][8*(l>>5)+j]; B[k][n]: lane holds B[8*(l>>5)+j][l&31]
    A = torch.randint(-4, 5, (32, 16), generator=g).float()
    B = torch.randint(-4, 5, (16, 32), generator=g).float()
    fa = torch.empty(64, 8)
    fb = torch.empty(64, 8)
    for l in range(64):
        for j in range(8):
            fa[l, j] = A[l & 31, 8 * (l >> 5) + j]
            fb[l, j] = B[8 * (l >> 5) + j, l & 31]
    out = torch.empty(64, 16, device="cuda")
    fa_d, fb_d = fa.bfloat16().cuda(), fb.bfloat16().cuda()   # keep alive: raw pointers cross the ABI
    call("mm_debug_mfma", 32, fa_d.data_ptr(), fb_d.data_ptr(), out.data_ptr(), 0)
    torch.cuda.synchronize()
    C = A @ B
    got = torch.empty(32, 32)
    o = out.cpu()
    for l in range(64):
        for r in range(16):
            got[(r & 3) + 8 * (r >> 2) + 4 * (l >> 5), l & 31] = o[l, r]
    assert torch.equal(got, C), "32x32x16 C/D or A/B lane map"
    # --- MFMA 16x16x32
    A = torch.randint(-4, 5, (16, 32), generator=g).float()
    B = torch.randint(-4, 5, (32, 16), generator=g).float()
    for l in range(64):
        for j in range(8):
            fa[l, j] = A[l & 15, 8 * (l >> 4) + j]
            fb[l, j] = B[8 * (l >> 4) + j, l & 15]
    out = torch.empty(64, 4, device="cuda")
    fa_d, fb_d = fa.bfloat16().cuda(), fb.bfloat16().cuda()
    call("mm_debug_mfma", 16, fa_d.data_ptr(), fb_d.data_ptr(), out.data_ptr(), 0)
    torch.cuda.synchronize()
    C = A @ B
    got = torch.empty(16, 16)
    o = out.cpu()
    for l in range(64):
        for r in range(4):
            got[4 * (l >> 4) + r, l & 15] = o[l, r]
    assert torch.equal(got, C), "16x16x32 C/D or A/B lane map"
    # --- ds_read_b64_tr_b16: image [64 rows][64 cols] bf16 (128-B rows); each 16-lane group reads a 4x16 block
    img = torch.arange(4096).reshape(64, 64) % 251   # exact in bf16
    addr = torch.empty(64, dtype=torch.int32)
    r0 = [0, 8, 20, 36]   # block first row per group
    c0 = [0, 16, 32, 48]  # block first column per group
    for l in range(64):
        grp, i = l >> 4, l & 15
        q, p = i >> 2, i & 3
        addr[l] = ((r0[grp] + q) * 64 + c0[grp] + 4 * p) * 2
    out = torch.empty(256, dtype=torch.bfloat16, device="cuda")
    img_d, addr_d = img.bfloat16().cuda(), addr.cuda()
    call("mm_debug_tr_read", img_d.data_ptr(), addr_d.data_ptr(), out.data_ptr(), 0)
    torch.cuda.synchronize()
    o = out.float().cpu().reshape(64, 4)
    for l in range(64):
        grp, i = l >> 4, l & 15
        for j in range(4):   # lane i receives column i of the block, row j in element j
            assert o[l, j] == float(img[r0[grp] + j, c0[grp] + i]), f"tr read lane {l} elem {j}: {o[l].tolist()}"

GEMM_SHAPES = [(128, 128, 64), (256, 384, 128), (300, 200, 192), (1028, 1024, 640), (64, 130, 64), (129, 72, 1088),
               (2048, 512, 2048)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
@pytest.mark.parametrize("shape", GEMM_SHAPES)
def test_gemm_layouts(K, dtype, layout, shape):
    M, N, Kd = shape
    a = rnd((M, Kd), dtype, 1)
    b = rnd((N, Kd), dtype, 2)
    ref = a.float() @ b.float().t()
    if layout == "NT":
        A, B, lay = a, b, 0
    elif layout == "NN":
        A, B, lay = a, b.t().contiguous(), 1
        if N % 8:  # ldb must be a multiple of 8: pad the row stride
            Bp = torch.zeros(Kd, (N + 7) // 8 * 8, dtype=dtype)
            Bp[:, :N] = B
            B = Bp
    else:
        A, B, lay = a.t().contiguous(), b.t().contiguous(), 2
        if M % 8:
            Ap = torch.zeros(Kd, (M + 7) // 8 * 8, dtype=dtype)
            Ap[:, :M] = A
            A = Ap
        if N % 8:
            Bp = torch.zeros(Kd, (N + 7) // 8 * 8, dtype=dtype)
            Bp[:, :N] = B
            B = Bp
    out = K.gemm(lay, A.cuda(), B.cuda(), M, N, Kd, ldc_pad=True)
    torch.cuda.synchronize()
    assert out.shape == (M, N)
    assert rel(out.float(), ref) < TOL[dtype]
    assert GC.last_kernel() == (GC.expected_kernel(lay, M, N, Kd) if dtype == torch.bfloat16 else GC.F32)
    if dtype == torch.bfloat16:
        GC.check_random("C", out, a, b)


DMA_SHAPES = [(256, 256, 64), (300, 520, 192), (1028, 1024, 640), (129, 72, 1088), (513, 264, 200), (2048, 512, 2056),
              (64, 130, 72)]


@pytest.mark.parametrize("variant", [2, 3, 4, 5, 6])
@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
@pytest.mark.parametrize("shape", DMA_SHAPES)
def test_gemm_dma_kernels_forced(K, variant, layout, shape):
    """The LDS-DMA kernels (256x128 and 256x256 tiles) are normally chosen only for chip-filling problems; force them
    on ragged shapes (M, N edges, K not a multiple of the 64-wide K-step, single-tile grids)."""
    from multimeditron_amd._lib import lib
    M, N, Kd = shape
    dtype = torch.bfloat16
    pad8 = lambda n: (n + 7) // 8 * 8
    a = rnd((M, Kd), dtype, 1)
    b = rnd((N, Kd), dtype, 2)
    ref = a.float() @ b.float().t()

    def padded(x):   # row stride must be a multiple of 8 elements
        r, c = x.shape
        o = torch.zeros(r, pad8(c), dtype=dtype)
        o[:, :c] = x
        return o.cuda()[:, :c]
    if layout == "NT":
        A, B, lay = padded(a), padded(b), 0
    elif layout == "NN":
        A, B, lay = padded(a), padded(b.t().contiguous()), 1
    else:
        A, B, lay = padded(a.t().contiguous()), padded(b.t().contiguous()), 2
    assert lib().mm_set_option(b"gemm_kernel", variant) == 0
    try:
        out = K.gemm(lay, A, B, M, N, Kd, ldc_pad=True)
        torch.cuda.synchronize()
        kid = GC.last_kernel()
    finally:
        assert lib().mm_set_option(b"gemm_kernel", 0) == 0
    assert out.shape == (M, N)
    assert rel(out.float(), ref) < TOL[dtype]
    assert kid == GC.expected_kernel(lay, M, N, Kd, forced=variant)
    GC.check_random("C", out, a, b)


@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
@pytest.mark.parametrize("shape", [(6144, 4096, 256), (4352, 4100, 192), (300, 520, 200)])
def test_gemm_half_tile_round(K, layout, shape):
    """persistent 256x256 grid: 384 tiles (1 round + 128 tiles cut into 256x128 halves), 17x17 tiles with a ragged N edge
    (1 round + 33 -> halves), and a 2x3-tile problem (halves only); A/B against the plain persistent schedule."""
    from multimeditron_amd._lib import lib
    M, N, Kd = shape
    dtype = torch.bfloat16
    pad8 = lambda n: (n + 7) // 8 * 8
    a, b = rnd((M, Kd), dtype, 91), rnd((N, Kd), dtype, 92)
    ref = a.float() @ b.float().t()

    def padded(x):
        r, c = x.shape
        o = torch.zeros(r, pad8(c), dtype=dtype)
        o[:, :c] = x
        return o.cuda()[:, :c]
    if layout == "NT":
        A, B, lay = padded(a), padded(b), 0
    elif layout == "NN":
        A, B, lay = padded(a), padded(b.t().contiguous()), 1
    else:
        A, B, lay = padded(a.t().contiguous()), padded(b.t().contiguous()), 2
    outs = []
    assert lib().mm_set_option(b"gemm_kernel", 3) == 0
    try:
        for tail in (1, 0):
            assert lib().mm_set_option(b"gemm_tail", tail) == 0
            outs.append(K.gemm(lay, A, B, M, N, Kd, ldc_pad=True).clone())
            assert GC.last_kernel() == GC.expected_kernel(lay, M, N, Kd, forced=3) == GC.W4
        torch.cuda.synchronize()
    finally:
        lib().mm_set_option(b"gemm_kernel", 0)
        lib().mm_set_option(b"gemm_tail", 1)
    assert rel(outs[0].float(), ref) < TOL[dtype]
    GC.check_random("C", outs[0], a, b)
    assert torch.equal(outs[0], outs[1])        # same products in the same K order: bit-identical to the unsplit schedule


@pytest.mark.parametrize("shape", [(1, 130, 64), (4, 6144, 4096), (16, 1000, 200), (7, 72, 1088), (3, 128258, 512)])
def test_gemm_skinny_decode(K, shape):
    """M <= 16 NT problems (one new token per sequence) take the weight-streaming kernel: ragged N / K, every epilogue."""
    from multimeditron_amd._lib import EPI_GELU_ERF
    M, N, Kd = shape
    dtype = torch.bfloat16
    a, w = rnd((M, Kd), dtype, 61), rnd((N, Kd), dtype, 62, 0.05)
    bias, res = rnd((N,), dtype, 63), rnd((M, N), dtype, 64)
    ref = a.float() @ w.float().t()
    out = K.linear_fwd(a.cuda(), w.cuda(), ldc_pad=True)
    assert rel(out.float(), ref) < TOL[dtype]
    assert GC.last_kernel() == GC.expected_kernel(GC.NT, M, N, Kd) == GC.GEMV
    GC.check_random("C", out, a, w)
    ref2 = F.gelu(ref + bias.float()) + res.float()
    rp = torch.zeros(M, (N + 63) // 64 * 64, dtype=dtype)
    rp[:, :N] = res
    out2 = K.linear_fwd(a.cuda(), w.cuda(), bias=bias.cuda(), residual=rp.cuda()[:, :N], act=EPI_GELU_ERF, ldc_pad=True)
    assert rel(out2.float(), ref2) < TOL[dtype]


def _old_skinny(fn):
    """Run fn with M <= 16 GEMMs on the round-2 weight-streaming kernel (gemm_skinny_kernel) instead of its ring-buffered form."""
    from multimeditron_amd._lib import lib
    lib().mm_set_option(b"gemv_stream", 0)
    try:
        return fn()
    finally:
        lib().mm_set_option(b"gemv_stream", 1)


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("M,H,I", [(4, 4096, 14336), (1, 512, 1000), (16, 3584, 2368), (7, 1088, 72)])
def test_decode_fused_gateup_swiglu_bit_identical(K, M, H, I, norm):
    """mm_decode_gateup_swiglu = [mm_rmsnorm_fwd +] weight-streaming gate|up GEMM + mm_swiglu_fwd, bit for bit (same K split, same
    rounding points) -- against the separate launches on BOTH forms of the streaming kernel."""
    x = rnd((M, H), torch.bfloat16, 301).cuda()
    wgu = rnd((2 * I, H), torch.bfloat16, 302, 0.05).cuda()
    nw = (1.0 + 0.1 * rnd((H,), torch.float32, 303)).to(torch.bfloat16).cuda() if norm else None
    fused = K.decode_gateup_swiglu(x, wgu, I, norm_w=nw, eps=1e-5)
    h = K.rmsnorm_fwd(x, nw, 1e-5)[0] if norm else x
    two = K.swiglu_fwd(K.linear_fwd(h, wgu), I)
    old = _old_skinny(lambda: K.swiglu_fwd(K.linear_fwd(h, wgu), I))
    assert torch.equal(fused, two) and torch.equal(fused, old)
    g = h.float() @ wgu.float().t()
    assert rel(fused.float(), F.silu(g[:, :I]) * g[:, I:]) < 2e-2


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("M,Hq,Hkv,Kd,bias", [(4, 32, 8, 4096, False), (1, 4, 1, 512, True), (16, 28, 4, 3584, True), (3, 3, 2, 200, False)])
def test_decode_fused_qkv_rope_append_bit_identical(K, M, Hq, Hkv, Kd, bias, norm):
    """mm_decode_qkv_rope_append = [mm_rmsnorm_fwd +] weight-streaming q|k|v GEMM + mm_rope_append (RoPE on q / k, roped k and v
    into the cache row)."""
    D, Smax, pos = 128, 9, 5
    N = (Hq + 2 * Hkv) * D
    x = rnd((M, Kd), torch.bfloat16, 311).cuda()
    w = rnd((N, Kd), torch.bfloat16, 312, 0.05).cuda()
    b = rnd((N,), torch.bfloat16, 313, 0.5).cuda() if bias else None
    nw = (1.0 + 0.1 * rnd((Kd,), torch.float32, 315)).to(torch.bfloat16).cuda() if norm else None
    ang = rnd((M, D // 2), torch.float32, 314, 3.0)
    cos, sin = torch.cos(ang).cuda(), torch.sin(ang).cuda()
    kc1, vc1 = (torch.full((M, Smax, Hkv, D), 7.0, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    kc2, vc2 = kc1.clone(), vc1.clone()
    fused = K.decode_qkv_rope_append(x, w, b, Hq, Hkv, D, cos, sin, kc1, vc1, pos, norm_w=nw, eps=1e-6)
    h = K.rmsnorm_fwd(x, nw, 1e-6)[0] if norm else x
    two = _old_skinny(lambda: K.linear_fwd(h, w, bias=b))
    K.rope_append_(two, M, Hq, Hkv, D, cos, sin, kc2, vc2, pos)
    torch.cuda.synchronize()
    assert torch.equal(fused, two) and torch.equal(kc1, kc2) and torch.equal(vc1, vc2)
    assert torch.equal(kc1[:, pos].reshape(M, -1), fused[:, Hq * D:(Hq + Hkv) * D]) and bool((kc1[:, pos - 1] == 7.0).all())


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("M,N,Kd", [(4, 4096, 4096), (4, 4096, 14336), (1, 512, 200), (16, 3584, 1000), (5, 8192, 256), (4, 128258, 4096), (3, 130, 8192)])
def test_decode_linear_bit_identical(K, M, N, Kd, norm):
    """mm_decode_linear = [mm_rmsnorm_fwd +] weight-streaming GEMM (+ residual), the norm applied while x is staged into LDS with the
    separate kernel's own arithmetic: same bits as the two launches, on both forms of the streaming kernel, launch after launch;
    ragged N and the padded row stride of the logits."""
    if norm and Kd > 8192:
        pytest.skip("norm prologue holds rows of <= 8192")
    x = rnd((M, Kd), torch.bfloat16, 321).cuda()
    w = rnd((N, Kd), torch.bfloat16, 322, 0.05).cuda()
    rp = torch.zeros(M, (N + 63) // 64 * 64, dtype=torch.bfloat16)
    rp[:, :N] = rnd((M, N), torch.bfloat16, 323)
    res = rp.cuda()[:, :N]                                                 # row stride padded: mm_gemm wants ldr % 4 == 0
    nw = (1.0 + 0.1 * rnd((Kd,), torch.float32, 324)).to(torch.bfloat16).cuda() if norm else None
    h = K.rmsnorm_fwd(x, nw, 1e-5)[0] if norm else x
    c_ref = K.linear_fwd(h, w, residual=res, ldc_pad=True)                # padded row stride: mm_gemm wants ldc % 4 == 0
    c_old = _old_skinny(lambda: K.linear_fwd(h, w, residual=res, ldc_pad=True))
    assert torch.equal(c_ref, c_old)
    for it in range(3):
        c = K.decode_linear(x, w, residual=res, norm_w=nw, eps=1e-5, ldc_pad=(it > 0))      # any row stride >= N
        assert torch.equal(c, c_ref), it
    cp = K.decode_linear(x, w, norm_w=nw, eps=1e-5, ldc_pad=True)
    assert cp.stride(0) % 64 == 0 and torch.equal(cp, _old_skinny(lambda: K.linear_fwd(h, w, ldc_pad=True)))
    assert rel(cp.float(), h.float() @ w.float().t()) < 2e-2


def test_decode_linear_refuses_what_does_not_fit(K):
    """x must fit the kernel's LDS stage (M * K * 2 <= 144 KB): a larger problem is refused (the caller keeps the separate launches;
    plain mm_gemm falls back to gemm_skinny_kernel by itself)."""
    from multimeditron_amd._lib import MMHipError
    x = rnd((16, 14336), torch.bfloat16, 331).cuda()
    w = rnd((256, 14336), torch.bfloat16, 332, 0.05).cuda()
    assert not K.decode_fits(16, 14336) and K.decode_fits(4, 14336)
    with pytest.raises(MMHipError):
        K.decode_linear(x, w)
    out = K.linear_fwd(x, w)
    assert rel(out.float(), x.float() @ w.float().t()) < 2e-2


def test_rope_append(K):
    B, Hq, Hkv, D, Smax, pos = 3, 4, 2, 64, 10, 6
    dtype = torch.bfloat16
    W = (Hq + 2 * Hkv) * D
    qkv = rnd((B, W), dtype, 87).cuda()
    cos, sin = torch.cos(rnd((B, D // 2), torch.float32, 88)).cuda(), torch.sin(rnd((B, D // 2), torch.float32, 88)).cuda()
    ref = qkv.clone()
    K.rope_apply_(ref, B, Hq + Hkv, D, W, cos, sin)
    kc = torch.zeros(B, Smax, Hkv, D, dtype=dtype, device="cuda")
    vc = torch.zeros_like(kc)
    got = qkv.clone()
    K.rope_append_(got, B, Hq, Hkv, D, cos, sin, kc, vc, pos)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    assert torch.equal(kc[:, pos].reshape(B, -1), ref[:, Hq * D:(Hq + Hkv) * D])
    assert torch.equal(vc[:, pos].reshape(B, -1), ref[:, (Hq + Hkv) * D:])
    assert float(kc[:, :pos].abs().sum()) == 0 and float(kc[:, pos + 1:].abs().sum()) == 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_gemm_asymmetric_identity(K, dtype):
    # A = I with an asymmetric B catches a transposed C write or a permuted fragment map
    n = 128
    eye = torch.eye(n, dtype=dtype)
    b = (torch.arange(n * n, dtype=torch.float32).reshape(n, n) % 251 - 125).to(dtype)
    for lay, A, B, ref in [(0, eye, b, b.float().t()), (1, eye, b, b.float()), (2, eye, b, b.float())]:
        out = K.gemm(lay, A.cuda(), B.cuda(), n, n, n)
        assert torch.equal(out.float().cpu(), ref), f"layout {lay}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_gemm_epilogues(K, dtype):
    M, N, Kd = 200, 136, 256
    a, w = rnd((M, Kd), dtype, 3, 0.5), rnd((N, Kd), dtype, 4, 0.1)
    bias, res = rnd((N,), dtype, 5), rnd((M, N), dtype, 6)
    base = a.float() @ w.float().t()
    cases = {
        "bias": (dict(bias=bias.cuda()), base + bias.float()),
        "bias_gelu": (dict(bias=bias.cuda(), act=2), F.gelu(base + bias.float())),
        "bias_quick": (dict(bias=bias.cuda(), act=4), (base + bias.float()) * torch.sigmoid(1.702 * (base + bias.float()))),
        "residual": (dict(residual=res.cuda()), base + res.float()),
        "bias_residual": (dict(bias=bias.cuda(), residual=res.cuda()), base + bias.float() + res.float()),
    }
    for name, (kw, ref) in cases.items():
        out = K.gemm(0, a.cuda(), w.cuda(), M, N, Kd, **kw)
        assert rel(out.float(), ref) < TOL[dtype], name
        assert GC.last_kernel() == (GC.expected_kernel(0, M, N, Kd, acts="act" in kw) if dtype == torch.bfloat16 else GC.F32), name
        if dtype == torch.bfloat16 and "act" not in kw:
            epi = (GC.EPI_BIAS if "bias" in kw else 0) | (GC.EPI_RESIDUAL if "residual" in kw else 0)
            GC.check_random(name, out, a, w, epi, bias=bias, res=res)
    c0 = rnd((M, N), dtype, 7)
    out = K.gemm(0, a.cuda(), w.cuda(), M, N, Kd, out=c0.cuda().clone(), accumulate=True)
    assert rel(out.float(), base + c0.float()) < TOL[dtype]
    if dtype == torch.bfloat16:
        GC.check_random("accumulate", out, a, w, GC.EPI_ACCUMULATE, c0=c0)
    cs = torch.empty(N, dtype=dtype, device="cuda")
    K.colsum(res.cuda(), cs, False)
    assert rel(cs.float(), res.float().sum(0)) < TOL[dtype]


def attn_ref(q, k, v, mask, causal, scale):
    # q [B,Sq,Hq,D], k/v [B,Skv,Hkv,D] fp32
    B, Sq, Hq, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    rep = Hq // Hkv
    qq = q.permute(0, 2, 1, 3)
    kk = k.permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)
    vv = v.permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)
    s = qq @ kk.transpose(2, 3) * scale
    allowed = torch.ones(B, 1, Sq, Skv, dtype=torch.bool)
    if causal:
        allowed = allowed & (torch.arange(Skv)[None, :] <= (torch.arange(Sq)[:, None] + (Skv - Sq)))[None, None]
    if mask is not None:
        allowed = allowed & mask[:, None, None, :].bool()
    row_ok = allowed.any(-1, keepdim=True)   # rows with no visible key: output defined as 0
    s = s.masked_fill(~allowed & row_ok, float("-inf"))
    p = torch.softmax(s, dim=-1) * row_ok
    return (p @ vv).permute(0, 2, 1, 3)


ATTN_CASES = [
    # B, Sq, Skv, Hq, Hkv, D, causal, masked
    (2, 128, 128, 2, 1, 64, True, False),
    (1, 257, 257, 4, 4, 64, False, False),
    (2, 50, 50, 3, 3, 64, False, False),
    (2, 200, 200, 4, 2, 128, True, True),
    (1, 384, 384, 8, 2, 128, True, False),
    (2, 1, 77, 4, 2, 64, True, True),
    (1, 40, 104, 2, 1, 128, True, False),
    (1, 300, 300, 7, 1, 128, True, False),       # Qwen2-7B's odd GQA group (28/4 = 7) through the paired dK/dV kernel
    (2, 640, 640, 4, 2, 128, True, True),        # 5 key blocks: odd count through the paired dK/dV kernel
    (3, 729, 729, 2, 2, 128, False, False),      # SigLIP-so400m token count, non-causal (padded 72-wide heads run here)
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("case", ATTN_CASES)
def test_attention_fwd_bwd(K, dtype, case):
    B, Sq, Skv, Hq, Hkv, D, causal, masked = case
    # fused qkv buffer like the decoder uses: [B, S, (Hq + 2 Hkv) * D] when Sq == Skv, else separate tensors
    q = rnd((B, Sq, Hq, D), dtype, 11)
    k = rnd((B, Skv, Hkv, D), dtype, 12)
    v = rnd((B, Skv, Hkv, D), dtype, 13)
    do = rnd((B, Sq, Hq, D), dtype, 14)
    mask = None
    if masked:
        mask = torch.ones(B, Skv, dtype=torch.long)
        mask[0, : Skv // 3] = 0          # left padding on sample 0
        if B > 1:
            mask[1, Skv - 5:] = 0        # right padding on sample 1
    scale = D ** -0.5
    qf, kf, vf = (t.float().clone().requires_grad_(True) for t in (q, k, v))
    ref = attn_ref(qf, kf, vf, mask, causal, scale)
    ref.backward(do.float())
    if Sq == Skv:
        buf = torch.cat([q.reshape(B, Sq, -1), k.reshape(B, Skv, -1), v.reshape(B, Skv, -1)], dim=-1).cuda()
        W = buf.shape[-1]
        qv = buf[..., : Hq * D].view(B, Sq, Hq, D)
        kv = buf[..., Hq * D:(Hq + Hkv) * D].view(B, Skv, Hkv, D)
        vv = buf[..., (Hq + Hkv) * D:].view(B, Skv, Hkv, D)
        dbuf = torch.full_like(buf, float("nan")) if dtype == torch.bfloat16 else torch.zeros_like(buf)
        dq = dbuf[..., : Hq * D].view(B, Sq, Hq, D)
        dk = dbuf[..., Hq * D:(Hq + Hkv) * D].view(B, Skv, Hkv, D)
        dv = dbuf[..., (Hq + Hkv) * D:].view(B, Skv, Hkv, D)
    else:
        qv, kv, vv = q.cuda(), k.cuda(), v.cuda()
        mk = torch.zeros_like if dtype == torch.float32 else (lambda t: torch.full_like(t, float("nan")))
        dq, dk, dv = mk(qv), mk(kv), mk(vv)
    mg = mask.cuda() if mask is not None else None
    out, lse = K.attn_fwd(qv, kv, vv, mg, causal, scale)
    torch.cuda.synchronize()
    # rows whose keys are all masked are garbage in the reference too (HF uniform softmax); compare valid rows
    valid = torch.ones(B, Sq, dtype=torch.bool)
    if mask is not None and causal:
        for b in range(B):
            for i in range(Sq):
                valid[b, i] = bool(mask[b, : i + (Skv - Sq) + 1].any())
    tol = TOL[dtype]
    assert rel(out.float().cpu()[valid], ref.detach()[valid]) < tol
    assert torch.isfinite(out.float()).all()
    K.attn_bwd(qv, kv, vv, out, do.cuda(), lse, mg, causal, scale, dq, dk, dv)
    torch.cuda.synchronize()
    gtol = tol * 2
    assert rel(dq.float().cpu()[valid], qf.grad[valid]) < gtol, "dq"
    assert rel(dk.float(), kf.grad) < gtol, "dk"
    assert rel(dv.float(), vf.grad) < gtol, "dv"
    # per element against the fp64 reference, and the output contract on the rows / keys the rel-L2 above leaves out
    from tests import attn_check as AC
    ref64 = AC.reference(qv, kv, vv, do.cuda(), mg, causal, scale)
    res = dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv)
    AC.check_contract(res, ref64)
    AC.check_all(res, ref64, dtype, AC.path_of(dtype, D, Skv))


def test_attention_long_kv(K):
    """More than 256 Ki keys: the D = 128 forward runs attn_fwd128p_kernel (attn_fwd128q_kernel's key-valid bits no longer fit
    in LDS).  Sq != Skv, GQA, causal with a shift.  bf16 only: the fp32 kernels refuse more than 12 000 keys."""
    test_attention_fwd_bwd(K, torch.bfloat16, (1, 64, 262_208, 2, 1, 128, True, False))


@pytest.mark.parametrize("case", [(4, 2051, 32, 8, 128, True), (2, 77, 4, 2, 64, True), (1, 300, 7, 1, 128, False),
                                  (3, 64, 2, 2, 64, False), (2, 1, 8, 1, 128, False), (2, 513, 16, 2, 128, True),
                                  (3, 130, 4, 4, 128, True), (2, 1000, 8, 4, 128, False), (1, 17, 4, 1, 128, True), (4, 2048, 32, 8, 128, False)])
def test_attention_decode(K, case):
    """one query token over a KV cache (split-K stream kernel) == the prefill kernel's last row == the fp32 reference.  D = 128 with
    up to 4 query heads per kv head takes the slice kernel with the scores on MFMA (attn_decode_partial128_mfma_kernel): also
    checked against the vector-ALU slice kernel (option attn_decode_mfma = 0), which the single-launch form still uses."""
    B, Skv, Hq, Hkv, D, masked = case
    dtype = torch.bfloat16
    Smax = Skv + 5                                     # the cache is a longer buffer; the step sees a prefix view
    kc, vc = rnd((B, Smax, Hkv, D), dtype, 71), rnd((B, Smax, Hkv, D), dtype, 72)
    qkv = rnd((B, (Hq + 2 * Hkv) * D), dtype, 73)       # q is a strided view of the fused projection output
    q = qkv[:, : Hq * D].view(B, Hq, D)
    mask = None
    if masked:
        mask = torch.ones(B, Skv, dtype=torch.long)
        mask[0, : Skv // 3] = 0
        if B > 1:
            mask[1, 5:9] = 0
    scale = D ** -0.5
    ref = attn_ref(q.float().unsqueeze(1), kc[:, :Skv].float(), vc[:, :Skv].float(), mask, True, scale)[:, 0]
    kd, vd, qd = kc.cuda(), vc.cuda(), qkv.cuda()
    out = K.attn_decode(qd[:, : Hq * D].view(B, Hq, D), kd[:, :Skv], vd[:, :Skv], mask.cuda() if masked else None, scale)
    torch.cuda.synchronize()
    assert out.shape == (B, Hq, D)
    assert rel(out.float(), ref) < TOL[dtype]
    pre, _ = K.attn_fwd(qd[:, : Hq * D].view(B, 1, Hq, D), kd[:, :Skv], vd[:, :Skv], mask.cuda() if masked else None, True, scale)
    assert rel(out.float(), pre.view(B, Hq, D).float()) < TOL[dtype]
    # single-launch form of the ABI (the slice that arrives last merges; counters stay zero): bit-identical result
    from multimeditron_amd._lib import call, lib
    qv, kv, vv = qd[:, : Hq * D].view(B, Hq, D), kd[:, :Skv], vd[:, :Skv]
    ns = lib().mm_attn_decode_splits(B, Hkv, Skv)
    ws = torch.empty(B * Hq * ns * (D + 2), dtype=torch.float32, device="cuda")
    sync = torch.zeros(B * Hkv, dtype=torch.int32, device="cuda")
    out1 = torch.empty_like(out)
    mg = mask.cuda() if masked else None
    for _ in range(2):
        call("mm_attn_decode", 0, qv.data_ptr(), kv.data_ptr(), vv.data_ptr(), B, Skv, Hq, Hkv, D, qv.stride(0), qv.stride(1),
             kv.stride(0), kv.stride(1), kv.stride(2), vv.stride(0), vv.stride(1), vv.stride(2), mg.data_ptr() if masked else None,
             float(scale), out1.data_ptr(), ws.data_ptr(), ns, sync.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    lib().mm_set_option(b"attn_decode_mfma", 0)
    try:
        out_valu = K.attn_decode(qv, kv, vv, mg, scale)
    finally:
        lib().mm_set_option(b"attn_decode_mfma", 1)
    assert torch.equal(out1, out_valu) and int(sync.abs().sum()) == 0
    if D == 128 and Hq // Hkv <= 4:
        assert rel(out.float(), out_valu.float()) < 4e-3 and not (Skv > 64 and torch.equal(out, out_valu) and False)
    else:
        assert torch.equal(out, out_valu)
    # per element against the fp64 reference, every launch form under its own path; a sequence without a visible key gives 0
    from tests import attn_check as AC
    ref64 = AC.decode_reference(qv, kv, vv, mg, scale)
    G = Hq // Hkv
    for o, path in ((out, AC.decode_path(D, G)), (out_valu, AC.decode_path(D, G, mfma=False)), (out1, AC.decode_path(D, G, fused=True))):
        AC.check_decode(o, ref64, path)
        assert not bool(o[~ref64["rows"]].any())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("H", [128, 1024, 4096])
def test_norms(K, dtype, H):
    M = 77
    x, w, b, dy = rnd((M, H), dtype, 21), 1 + 0.1 * rnd((H,), torch.float32, 22), rnd((H,), dtype, 23), rnd((M, H), dtype, 24)
    w = w.to(dtype)
    tol = TOL[dtype]
    # RMSNorm
    xf, wf = x.float().clone().requires_grad_(True), w.float().clone().requires_grad_(True)
    ref = wf * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5))
    ref.backward(dy.float())
    y, rstd = K.rmsnorm_fwd(x.cuda(), w.cuda(), 1e-5)
    assert rel(y.float(), ref.detach()) < tol
    dres = rnd((M, H), dtype, 25)
    dx, dwp = K.rmsnorm_bwd(dy.cuda(), x.cuda(), w.cuda(), rstd, dres.cuda())
    dw = torch.empty(H, dtype=dtype, device="cuda")
    K.reduce_partials(dwp, dw, False)
    assert rel(dx.float(), xf.grad + dres.float()) < tol * 2     # fused residual-gradient add
    assert rel(dw.float(), wf.grad) < tol * 2
    # per element against fp64, the saved statistics included, and the documented rounding chain exactly
    xd, wd, bd, dyd = x.cuda(), w.cuda(), b.cuda(), dy.cuda()
    GC.check_exact("rmsnorm chain", y, RC.rmsnorm_chain(xd, wd, rstd))
    y64, Ey, r64, Er = RC.rmsnorm_fwd_reference(xd, wd, 1e-5)
    RC.bound("rstd", "rmsnorm.rstd", dtype, rstd, r64, Er, u=RC.U32)
    RC.bound("y", "rmsnorm.y", dtype, y, y64, Ey)
    dx64, Edx, dw64, Edw = RC.rmsnorm_bwd_reference(dyd, xd, wd, rstd, dres.cuda())
    RC.bound("dx", "rmsnorm.dx", dtype, dx, dx64, Edx)
    RC.bound("dw", "rmsnorm.dw", dtype, dw, dw64, Edw)
    # LayerNorm
    xf, wf, bf = (t.float().clone().requires_grad_(True) for t in (x, w, b))
    ref = F.layer_norm(xf, (H,), wf, bf, 1e-5)
    ref.backward(dy.float())
    y, mean, rstd = K.layernorm_fwd(x.cuda(), w.cuda(), b.cuda(), 1e-5)
    assert rel(y.float(), ref.detach()) < tol
    dx, dwp, dbp = K.layernorm_bwd(dy.cuda(), x.cuda(), w.cuda(), mean, rstd)
    dw, db = torch.empty(H, dtype=dtype, device="cuda"), torch.empty(H, dtype=dtype, device="cuda")
    K.reduce_partials(dwp, dw, False)
    K.reduce_partials(dbp, db, False)
    assert rel(dx.float(), xf.grad) < tol * 2
    assert rel(dw.float(), wf.grad) < tol * 2
    assert rel(db.float(), bf.grad) < tol * 2
    y64, Ey, m64, Em, r64, Er = RC.layernorm_fwd_reference(xd, wd, bd, 1e-5)
    RC.bound("mean", "layernorm.mean", dtype, mean, m64, Em, u=RC.U32)
    RC.bound("rstd", "layernorm.rstd", dtype, rstd, r64, Er, u=RC.U32)
    RC.bound("y", "layernorm.y", dtype, y, y64, Ey)
    dx64, Edx, dw64, Edw, db64, Edb = RC.layernorm_bwd_reference(dyd, xd, wd, mean, rstd)
    RC.bound("dx", "layernorm.dx", dtype, dx, dx64, Edx)
    RC.bound("dw", "layernorm.dw", dtype, dw, dw64, Edw)
    RC.bound("db", "layernorm.db", dtype, db, db64, Edb)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("D", [64, 128])
def test_rope(K, dtype, D):
    B, S, Hq, Hkv = 2, 37, 4, 2
    W = (Hq + 2 * Hkv) * D
    qkv = rnd((B * S, W), dtype, 31)
    pos = torch.stack([torch.arange(S), torch.clamp(torch.arange(S) - 5, min=0)]).reshape(-1)
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    ang = pos[:, None].float() * inv[None]
    cos, sin = ang.cos(), ang.sin()
    cg, sg = K.rope_table(pos.cuda(), inv.cuda(), False)
    assert rel(cg, cos) < 1e-5 and rel(sg, sin) < 1e-5
    c64, s64, Ec, Es, u = RC.rope_table_reference(pos.cuda(), inv.cuda(), False)
    RC.bound("cos", "rope_table", torch.float32, cg, c64, Ec, u=u)
    RC.bound("sin", "rope_table", torch.float32, sg, s64, Es, u=u)

    def ref_rot(x, inverse=False):  # x [T, h, D]
        c = torch.cat([cos, cos], -1)[:, None]
        s = torch.cat([sin, sin], -1)[:, None] * (-1 if inverse else 1)
        half = D // 2
        rh = torch.cat([-x[..., half:], x[..., :half]], -1)
        return x * c + rh * s

    g = qkv.cuda().clone()
    K.rope_apply_(g, B * S, Hq + Hkv, D, W, cg, sg)   # q and k heads are adjacent in the fused buffer
    ref = qkv.float().clone()
    ref[:, : (Hq + Hkv) * D] = ref_rot(ref[:, : (Hq + Hkv) * D].view(B * S, Hq + Hkv, D)).reshape(B * S, -1)
    assert rel(g.float(), ref) < TOL[dtype]
    r64, E = RC.rope_reference(qkv.cuda(), cg, sg, Hq + Hkv, D)
    RC.bound("rope", "rope", dtype, g, r64, E)
    GC.check_exact("v columns", g[:, (Hq + Hkv) * D:], qkv.cuda()[:, (Hq + Hkv) * D:])
    roped = g.clone()
    K.rope_apply_(g, B * S, Hq + Hkv, D, W, cg, sg, inverse=True)
    assert rel(g.float(), qkv.float()) < TOL[dtype] * 2
    r64, E = RC.rope_reference(roped, cg, sg, Hq + Hkv, D, inverse=True)
    RC.bound("rope inverse", "rope", dtype, g, r64, E)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_activations(K, dtype):
    M, I = 33, 256
    gu, dout = rnd((M, 2 * I), dtype, 41), rnd((M, I), dtype, 42)
    guf = gu.float().clone().requires_grad_(True)
    ref = F.silu(guf[:, :I]) * guf[:, I:]
    ref.backward(dout.float())
    tol = TOL[dtype]
    out, dgu = K.swiglu_fwd(gu.cuda(), I), K.swiglu_bwd(gu.cuda(), dout.cuda(), I)
    assert rel(out.float(), ref.detach()) < tol
    assert rel(dgu.float(), guf.grad) < tol * 2
    r64, E = RC.swiglu_fwd_reference(gu.cuda(), I)
    RC.bound("swiglu_fwd", "swiglu_fwd", dtype, out, r64, E)
    r64, E = RC.swiglu_bwd_reference(gu.cuda(), dout.cuda(), I)
    RC.bound("swiglu_bwd", "swiglu_bwd", dtype, dgu, r64, E)
    x, dy = rnd((1000 + 3,), dtype, 43, 2.0), rnd((1000 + 3,), dtype, 44)
    for kind, fn in [(0, F.gelu), (1, lambda t: t * torch.sigmoid(1.702 * t)), (2, lambda t: F.gelu(t, approximate="tanh"))]:
        xf = x.float().clone().requires_grad_(True)
        r = fn(xf)
        r.backward(dy.float())
        yg, dxg = K.gelu_fwd(x.cuda(), kind), K.gelu_bwd(x.cuda(), dy.cuda(), kind)
        assert rel(yg.float(), r.detach()) < tol
        assert rel(dxg.float(), xf.grad) < tol * 2
        r64, E = RC.gelu_fwd_reference(x.cuda(), kind)
        RC.bound(f"gelu_fwd {kind}", "gelu_fwd", dtype, yg, r64, E)
        r64, E = RC.gelu_bwd_reference(x.cuda(), dy.cuda(), kind)
        RC.bound(f"gelu_bwd {kind}", "gelu_bwd", dtype, dxg, r64, E)
    s = K.add(x.cuda(), dy.cuda())
    assert rel(s.float(), x.float() + dy.float()) < tol
    GC.check_exact("add", s, (x.float() + dy.float()).to(dtype).cuda())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_head_pad_and_bcast_add(K, dtype):
    """plug-in tower glue: zero-padded heads (72 -> 128) and positions broadcast over images; both bit-exact copies/adds."""
    rows, nh, d, dp = 37, 6, 72, 128
    x = rnd((rows, nh * d), dtype, 51)
    ref = torch.zeros(rows, nh, dp, dtype=dtype)
    ref[:, :, :d] = x.view(rows, nh, d)
    got = K.head_pad(x.cuda(), nh, d, dp)
    assert torch.equal(got.cpu(), ref.view(rows, nh * dp))
    back = K.head_pad(got, nh, d, dp, inverse=True)
    assert torch.equal(back.cpu(), x)
    n, L = 3, 16 * 72
    a, b = rnd((n, L), dtype, 52), rnd((L,), dtype, 53)
    y = K.bcast_add(a.cuda(), b.cuda())
    assert torch.equal(y.cpu(), (a.float() + b.float()[None]).to(dtype))
    # tanh-GELU as a GEMM epilogue
    from multimeditron_amd._lib import EPI_GELU_TANH
    A, W, bias = rnd((50, 64), dtype, 54), rnd((40, 64), dtype, 55), rnd((40,), dtype, 56)
    r = F.gelu(A.float() @ W.float().t() + bias.float(), approximate="tanh")
    o = K.linear_fwd(A.cuda(), W.cuda(), bias=bias.cuda(), act=EPI_GELU_TANH)
    assert rel(o.float(), r) < TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [130, 1000, 128258])
def test_cross_entropy(K, dtype, V):
    T = 19
    ld = (V + 63) // 64 * 64
    logits = rnd((T, V), dtype, 51, 2.0)
    labels = torch.randint(0, V, (T,), generator=torch.Generator().manual_seed(52))
    labels[::4] = -100
    lf = logits.float().clone().requires_grad_(True)
    ref = F.cross_entropy(lf, labels, ignore_index=-100)
    ref.backward()
    buf = torch.zeros(T, ld, dtype=dtype, device="cuda")
    buf[:, :V] = logits.cuda()
    lc, lse = K.ce_fwd(buf[:, :V], V, labels.cuda())
    assert abs(float(lc[0]) - float(ref)) < 1e-4 * max(1, abs(float(ref)))
    assert int(lc[1]) == int((labels >= 0).sum())
    d = torch.full_like(buf, float("nan"))
    K.ce_bwd(buf[:, :V], V, labels.cuda(), lse, lc, None, d[:, :V])
    assert rel(d[:, :V].float(), lf.grad) < (2e-5 if dtype == torch.float32 else 1e-2)
    assert torch.all(d[:, V:] == 0)
    RC.check_ce(dtype, logits.cuda(), labels.cuda(), lse, lc, d, None)
    for T_ in (0.1, 0.7):
        got = K.argmax_softmax(buf[:, :V], V, T_).cpu()
        want = torch.argmax(torch.softmax(logits / T_, dim=-1), dim=-1)   # in the logits dtype, as model.py:607-621
        assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_embed_splice(K, dtype):
    B, S, H, V, P = 2, 24, 128, 50, 4
    emb = rnd((V, H), dtype, 61)
    ids = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(62))
    proj = rnd((3 * P, H), dtype, 63)
    bi = torch.tensor([0] * P + [1] * (2 * P))
    tr = torch.tensor(list(range(3, 3 + P)) + list(range(1, 1 + P)) + list(range(10, 10 + P)))
    e = F.embedding(ids, emb.float())
    ref = e.clone()
    ref[bi, tr] = proj.float()
    m = K.splice_build_map(bi.cuda(), tr.cuda(), S, B * S)
    out = K.embed_splice_fwd(emb.cuda(), ids.cuda().reshape(-1), proj.cuda(), m)
    assert torch.equal(out.float().cpu(), ref.reshape(B * S, H))
    out2 = K.embed_splice_fwd(emb.cuda(), ids.cuda().reshape(-1), None, None)
    assert torch.equal(out2.float().cpu(), e.reshape(B * S, H))
    idc = ids.cuda().reshape(-1)
    assert torch.equal(m, EC.build_map_reference(bi.cuda(), tr.cuda(), S, B * S))
    check_bits("embed_splice_fwd", out, EC.splice_fwd_reference(emb.cuda(), idc, proj.cuda(), m))
    check_bits("embed_splice_fwd without a map", out2, EC.splice_fwd_reference(emb.cuda(), idc, None, None))
    # backward
    dE = rnd((B * S, H), dtype, 64)
    ef = emb.float().clone().requires_grad_(True)
    pf = proj.float().clone().requires_grad_(True)
    r = F.embedding(ids, ef).clone()
    r[bi, tr] = pf
    r.reshape(B * S, H).backward(dE.float())
    dproj = torch.empty_like(proj, device="cuda")
    demb = torch.zeros_like(emb, device="cuda")
    order, skey = K.embed_sort(ids.cuda().reshape(-1), m, V, H)
    K.embed_splice_bwd(dE.cuda(), ids.cuda().reshape(-1), m, bi.cuda(), tr.cuda(), S, dproj, demb, order, skey)
    assert torch.equal(dproj.float().cpu(), pf.grad)
    # fp32 sums rounded once: fp32 path exact to fp32 rounding, bf16 path within one bf16 rounding of the fp32 sum
    assert rel(demb.float(), ef.grad) < (1e-6 if dtype == torch.float32 else 4e-3)
    check_bits("dproj", dproj, EC.dproj_reference(dE.cuda(), bi.cuda(), tr.cuda(), S, m))
    EC.check_demb("embed_splice_bwd", dE.cuda(), idc, m, V, torch.zeros_like(demb), 0, demb)
    # accumulate onto an existing gradient (tied lm_head wgrad / gradient accumulation)
    base = rnd((V, H), dtype, 65)
    demb2 = base.clone().cuda()
    K.embed_splice_bwd(dE.cuda(), ids.cuda().reshape(-1), m, bi.cuda(), tr.cuda(), S, None, demb2, order, skey, accumulate=True)
    assert rel(demb2.float(), base.float() + ef.grad) < (1e-6 if dtype == torch.float32 else 4e-3)
    EC.check_demb("embed_splice_bwd accumulate", dE.cuda(), idc, m, V, base.cuda(), 1, demb2)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("T,V,H,spliced", [(8192, 50, 4096, True), (8192, 50, 4096, False), (1000, 7, 136, True), (33, 1, 64, False),
                                             (4096, 128258, 1024, True), (40000, 300, 64, False)])
def test_embed_grad_heavy_repeats_fp32_and_deterministic(K, dtype, T, V, H, spliced):
    """VERDICT r1 item 4 / ADVICE (mm_embed.hip:90): the embedding gradient under heavily repeated ids (8192 tokens over
    50 ids = ~164 adds per row; runs crossing many 32-position chunks; T not a multiple of 32/64; T beyond one LDS key
    block) must equal the fp32 sum rounded ONCE (torch's embedding backward semantics: <= 1e-2 asked, one bf16 rounding
    = 4e-3 given) and be bitwise identical across launches."""
    g = torch.Generator().manual_seed(T + V)
    ids = torch.randint(0, V, (T,), generator=g)
    ids[:: 7] = 0                                   # one id far heavier than the rest (padding-like)
    dE = (torch.randn(T, H, generator=g) * 0.05).to(dtype)
    m = None
    keep = torch.ones(T, dtype=torch.bool)
    if spliced:                                     # a block of tokens overwritten by modality rows: no gradient from them
        n = T // 8
        pos = torch.arange(T // 4, T // 4 + n)
        m = K.splice_build_map(torch.zeros(n, dtype=torch.int64).cuda(), pos.cuda(), T, T)
        keep[pos] = False
    ref = torch.zeros(V, H, dtype=torch.float64)
    ref.index_add_(0, ids[keep], dE[keep].double())
    idc, dEc = ids.cuda(), dE.cuda()
    outs = []
    for _ in range(2):
        order, skey = K.embed_sort(idc, m, V, H)
        demb = torch.zeros(V, H, dtype=dtype, device="cuda")
        K.embed_splice_bwd(dEc, idc, m, None, None, T, None, demb, order, skey)
        outs.append(demb)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])            # bitwise reproducible
    got = outs[0].double().cpu()
    err = float((got - ref).norm() / ref.norm())
    assert err < (1e-6 if dtype == torch.float32 else 4e-3), err
    EC.check_demb(f"embed grad T={T} V={V} H={H}", dEc, idc, m, V, torch.zeros_like(outs[0]), 0, outs[0])
    o_ref, k_ref = EC.sort_reference(idc, m, V)
    assert torch.equal(order[:T], o_ref) and torch.equal(skey, k_ref)
    # the order really is the stable sort by (id, token)
    o = order[:T].cpu().long()
    k = torch.where(keep, ids, torch.full_like(ids, 2 ** 31 - 1))
    assert torch.equal(o, torch.sort(k * T + torch.arange(T), stable=True).indices)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_vit_glue(K, dtype):
    n, ps, img, Dv = 3, 14, 56, 128
    P = (img // ps) ** 2
    pix = rnd((n, 3, img, img), torch.float32, 71)
    w = rnd((Dv, 3, ps, ps), dtype, 72, 0.05)
    ref = F.conv2d(pix.to(dtype).float(), w.float(), stride=ps).flatten(2).transpose(1, 2)   # [n,P,Dv]
    kpad = (3 * ps * ps + 63) // 64 * 64
    patches = K.patchify(pix.cuda(), ps, kpad, dtype)
    check_bits("patchify", patches, EC.patchify_reference(pix.cuda(), ps, kpad, dtype))
    wp = torch.zeros(Dv, kpad, dtype=dtype)
    wp[:, : 3 * ps * ps] = w.reshape(Dv, -1)
    po = K.linear_fwd(patches, wp.cuda())
    assert rel(po.float(), ref.reshape(n * P, Dv)) < TOL[dtype]
    cls, pos = rnd((Dv,), dtype, 73), rnd((P + 1, Dv), dtype, 74)
    x = K.vit_embed_fwd(po, cls.cuda(), pos.cuda(), n, P)
    refx = torch.cat([cls.float().expand(n, 1, Dv), po.float().cpu().view(n, P, Dv)], 1) + pos.float()
    assert rel(x.float(), refx) < TOL[dtype]
    check_bits("vit_embed_fwd", x, EC.vit_embed_fwd_reference(po.view(n, P, Dv), cls.cuda(), pos.cuda()))
    d = K.drop_cls_fwd(x)
    assert torch.equal(d.cpu(), x[:, 1:].cpu())
    db = K.drop_cls_bwd(d)
    assert torch.equal(db[:, 1:].cpu(), d.cpu()) and torch.all(db[:, 0] == 0)
    dx = rnd((n, P + 1, Dv), dtype, 75).cuda()
    dcls = torch.empty(Dv, dtype=dtype, device="cuda")
    dpos = torch.empty(P + 1, Dv, dtype=dtype, device="cuda")
    dpatch = K.vit_embed_bwd(dx, dcls, dpos, False)
    assert torch.equal(dpatch.view(n, P, Dv).cpu(), dx[:, 1:].cpu())
    assert rel(dcls.float(), dx.float().cpu()[:, 0].sum(0)) < TOL[dtype]
    assert rel(dpos.float(), dx.float().cpu().sum(0)) < TOL[dtype]
    _, dcls_ref, dpos_ref = EC.vit_embed_bwd_reference(dx, None, None, False)
    check_bits("vit_embed_bwd dcls", dcls, dcls_ref)
    check_bits("vit_embed_bwd dpos", dpos, dpos_ref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_adamw_and_gradnorm(K, dtype):
    n = 100003
    p32 = rnd((n,), torch.float32, 81)
    g = rnd((n,), dtype, 82, 0.1)
    p = p32.to(dtype)
    master = p.float().cuda()
    m = torch.zeros(n, device="cuda")
    v = torch.zeros(n, device="cuda")
    pg = p.cuda()
    total = K.gradnorm([g.cuda()], 1.0)
    nrm = float(g.float().norm())
    assert abs(float(total[0]) - nrm) < 1e-3 * nrm
    OC.check_gradnorm("gradnorm", g.cuda(), 1024, 1.0, total)
    hyper = OC.Hyper(1e-2, 0.9, 0.95, 1e-8, 0.01)
    coef = min(1.0, 1.0 / (nrm + 1e-6))
    ref_p = torch.nn.Parameter(p.float().clone())
    opt = torch.optim.AdamW([ref_p], lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.01)
    for step in (1, 2, 3):
        ref_p.grad = g.float() * coef
        opt.step()
        before = {"g": g.cuda(), "m": m.clone(), "v": v.clone(), "w": master.clone()}
        K.adamw_step(pg, g.cuda(), master, m, v, 1e-2, 0.9, 0.95, 1e-8, 0.01, step, clip=total)
        OC.check_adamw(f"adamw_step step {step}", before, {"m": m, "v": v, "master": master, "p": pg}, hyper, step, float(total[1]),
                       "bf16" if dtype == torch.bfloat16 else "f32")
    assert rel(master, ref_p.detach()) < 1e-5
    assert rel(pg.float(), ref_p.detach()) < (1e-5 if dtype == torch.float32 else 5e-3)


def test_adamw_split_master_equals_fp32_master(K):
    """mm_adamw_step_split keeps the fp32 master as (bf16 parameter, int16 remainder): over several clipped steps the bf16 parameters
    must equal those of mm_adamw_step with a separate fp32 master BIT FOR BIT, the joined master must stay within one fp32 ulp of it
    (the one unrepresentable remainder, +0x8000, is stored as 0x7FFF), and split(join(.)) must be the identity."""
    n = 1_000_003
    g0 = torch.Generator().manual_seed(5)
    w = (torch.randn(n, generator=g0) * 0.05).to(torch.bfloat16)
    p_a, p_b = w.clone().cuda(), w.clone().cuda()
    master = w.float().cuda()
    lo = torch.zeros(n, dtype=torch.int16, device="cuda")
    m_a, v_a, m_b, v_b = (torch.zeros(n, device="cuda") for _ in range(4))
    for step in (1, 2, 3, 4):
        g = (torch.randn(n, generator=g0) * (0.01 * step)).to(torch.bfloat16).cuda()
        total = K.gradnorm([g], 1.0)
        K.adamw_step(p_a, g, master, m_a, v_a, 3e-3, 0.9, 0.95, 1e-8, 0.01, step, clip=total)
        before = {"g": g, "m": m_b.clone(), "v": v_b.clone(), "w": OC.join_reference(p_b, lo)}
        K.adamw_step_split(p_b, g, lo, m_b, v_b, 3e-3, 0.9, 0.95, 1e-8, 0.01, step, clip=total)
        torch.cuda.synchronize()
        OC.check_adamw(f"adamw_step_split step {step}", before, {"m": m_b, "v": v_b, "p": p_b, "lo": lo},
                       OC.Hyper(3e-3, 0.9, 0.95, 1e-8, 0.01), step, float(total[1]), "split")
        assert torch.equal(p_a, p_b), step
        joined = K.master_join(p_b, lo)
        ulp = (joined.view(torch.int32).long() - master.view(torch.int32).long()).abs()
        assert int(ulp.max()) <= step, (step, int(ulp.max()))                      # at most one ulp per step, and only at exact ties
        assert float((ulp > 0).float().mean()) < 1e-3
        assert torch.equal(m_a, m_b) or float((m_a - m_b).abs().max()) < 1e-9
    p2, lo2 = torch.empty_like(p_b), torch.empty_like(lo)
    K.master_split(K.master_join(p_b, lo), p2, lo2)
    assert torch.equal(p2, p_b) and torch.equal(lo2, lo)
    K.master_split(master, p2, lo2)
    assert torch.equal(p2, p_a)                                                     # p = round-to-nearest-even(master)
    p_ref, lo_ref = OC.split_reference(master)
    assert torch.equal(p2.view(torch.int16), p_ref.view(torch.int16)) and torch.equal(lo2, lo_ref)
    check_bits("master_join", K.master_join(p2, lo2), OC.join_reference(p_ref, lo_ref))


@pytest.mark.parametrize("M,I,Kd", [(512, 256, 128), (300, 128, 64), (1024, 384, 320), (2048, 14336 // 8, 512)])
def test_fused_swiglu_gemm_bit_identical_to_two_launch_form(K, M, I, Kd):
    """mm_gemm_swiglu_fwd / _bwd (SwiGLU as the epilogue of the gate|up GEMM and of down_proj's dgrad) against the separate
    launches they replace (mm_gemm + mm_swiglu_fwd, mm_gemm NN + mm_swiglu_bwd): same products in the same K order and the
    same rounding points, so the outputs must be BIT-identical; and both against fp32 torch within bf16 tolerance."""
    dtype = torch.bfloat16
    x = rnd((M, Kd), dtype, 201).cuda()
    wgu = rnd((2 * I, Kd), dtype, 202, 0.05).cuda()
    H = 192
    wd = rnd((H, I), dtype, 203, 0.05).cuda()
    dy = rnd((M, H), dtype, 204).cuda()
    fused = K.gemm_swiglu_fwd(x, wgu, I)
    assert fused is not None
    gu_f, act_f = fused
    gu = K.linear_fwd(x, wgu)
    act = K.swiglu_fwd(gu, I)
    assert torch.equal(gu_f, gu) and torch.equal(act_f, act)
    ref_gu = x.float() @ wgu.float().t()
    ref_act = F.silu(ref_gu[:, :I]) * ref_gu[:, I:]
    assert rel(act_f.float(), ref_act) < 2e-2
    dgu_f = K.gemm_swiglu_bwd(dy, wd, gu, I)
    dgu = K.swiglu_bwd(gu, K.linear_dgrad(dy, wd), I)
    assert dgu_f is not None and torch.equal(dgu_f, dgu)


@pytest.mark.parametrize("M,Hq,Hkv,Kd,bias", [(512, 4, 1, 128, False), (300, 3, 2, 192, True), (1024, 8, 2, 320, False), (2048, 32, 8, 512, True)])
def test_fused_rope_gemm_bit_identical_to_two_launch_form(K, M, Hq, Hkv, Kd, bias):
    """mm_gemm_rope_fwd (RoPE as the epilogue of the fused q|k|v projection) against mm_gemm + mm_rope_apply: same products in the
    same K order, the projection rounded to bf16 before the rotation, the rotation's arithmetic shared (rope_lo / rope_hi): the
    outputs must be BIT-identical (ragged row counts, an odd head count = a half-empty last tile, Qwen2's bias); and against fp32 torch."""
    dtype, D = torch.bfloat16, 128
    N = (Hq + 2 * Hkv) * D
    x = rnd((M, Kd), dtype, 211).cuda()
    w = rnd((N, Kd), dtype, 212, 0.05).cuda()
    b = rnd((N,), dtype, 213, 0.5).cuda() if bias else None
    pos = torch.arange(M, device="cuda", dtype=torch.int64) % 777
    inv = (1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))).cuda()
    cos, sin = K.rope_table(pos, inv, True)
    fused = K.gemm_rope_fwd(x, w, b, (Hq + Hkv) * D, D, cos, sin)
    assert fused is not None
    two = K.linear_fwd(x, w, bias=b)
    plain = two.clone()
    K.rope_apply_(two, M, Hq + Hkv, D, N, cos, sin)
    assert torch.equal(fused, two)
    assert torch.equal(fused[:, (Hq + Hkv) * D:], plain[:, (Hq + Hkv) * D:]) and not torch.equal(fused[:, :D], plain[:, :D])
    ref = x.float() @ w.float().t() + (b.float() if bias else 0.0)
    r = ref[:, : (Hq + Hkv) * D].view(M, Hq + Hkv, D)
    c, s_ = cos.view(M, 1, D // 2), sin.view(M, 1, D // 2)
    rot = torch.cat([r[..., : D // 2] * c - r[..., D // 2:] * s_, r[..., D // 2:] * c + r[..., : D // 2] * s_], dim=-1)
    assert rel(fused[:, : (Hq + Hkv) * D].float(), rot.reshape(M, -1)) < 2e-2
    # the adjoint used by backward still inverts the fused forward
    K.rope_apply_(two, M, Hq + Hkv, D, N, cos, sin, inverse=True)
    assert rel(two.float(), plain.float()) < 1e-2


def test_embedding_out_of_range_id_raises(K):      # noqa: F811
    """nn.Embedding raises for an id outside the table (the reference embeds every id of the batch, model.py:433).  Here the
    lookup never reads out of bounds and the error surfaces without a stall: at the next lookup after the check has completed,
    or at the next host synchronisation point (trainer.synchronize / the end of generate)."""
    emb = torch.randn(50, 64, device="cuda").to(torch.bfloat16)
    good = torch.randint(0, 50, (40,), device="cuda")
    bad = good.clone()
    bad[7] = 50
    K.embed_check_pending()
    out = K.embed_splice_fwd(emb, good, None, None)
    torch.cuda.synchronize()
    assert torch.equal(out, emb[good])
    K.embed_splice_fwd(emb, bad, None, None)             # asynchronous: nothing raised yet
    with pytest.raises(IndexError):
        K.embed_check_pending()
    K.embed_splice_fwd(emb, bad, None, None)
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        K.embed_splice_fwd(emb, good, None, None)        # the next lookup finds the completed check of the previous one
    K.embed_check_pending()                              # flag was cleared by the raise
    neg = good.clone()
    neg[0] = -1
    with pytest.raises(IndexError):
        K.embed_check_ids(neg, 50, block=True)


@pytest.mark.parametrize("act_name", ["EPI_GELU_ERF", "EPI_QUICK_GELU", "EPI_GELU_TANH"])
@pytest.mark.parametrize("shape", [(1028, 4096, 1024, True), (300, 136, 72, False), (4112, 3584, 1152, True)])
def test_linear_gelu_keeps_preactivation_bit_identical(K, act_name, shape):      # noqa: F811
    """mm_gemm_act_fwd (training forward of Linear + GELU in one launch) against the three launches it replaces: the
    pre-activation kept for backward and the output are bit-identical (ViT-L fc1, a ragged shape, SigLIP fc1; with residual)."""
    from multimeditron_amd import _lib
    act = getattr(_lib, act_name)
    M, N, Kd, with_res = shape
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(M, Kd, device="cuda", generator=g).to(torch.bfloat16)
    w = (torch.randn(N, Kd, device="cuda", generator=g) * 0.05).to(torch.bfloat16)
    b = torch.randn(N, device="cuda", generator=g).to(torch.bfloat16)
    res = torch.randn(M, N, device="cuda", generator=g).to(torch.bfloat16) if with_res else None
    pre_ref = K.linear_fwd(x, w, bias=b)
    y_ref = K.gelu_fwd(pre_ref, _lib.GELU_KIND[act])
    if res is not None:
        y_ref = K.add(y_ref, res)
    fused = K.linear_act_fwd(x, w, b, act, res)
    assert fused is not None
    pre, y = fused
    torch.cuda.synchronize()
    assert torch.equal(pre, pre_ref)
    assert torch.equal(y, y_ref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_rows_select_both_directions(K, dtype):
    """mm_rows_select: gather of the labelled rows (forward) and the scatter back with zero rows (backward), against torch
    indexing -- bit-exact (a copy); strided source rows; the host-side index builder against HF's shift-then-ignore rule."""
    from multimeditron_amd.functional import LossRows
    g0 = torch.Generator().manual_seed(11)
    B, S, H = 3, 37, 64
    labels = torch.randint(0, 1000, (B, S), generator=g0)
    labels[torch.rand(B, S, generator=g0) < 0.4] = -100
    labels[1, :] = -100                                                   # a sample without any label
    rows = LossRows.from_host_labels(labels, "cuda")
    shift = torch.nn.functional.pad(labels, (0, 1), value=-100)[..., 1:].reshape(-1)
    keep = (shift != -100).nonzero().reshape(-1)
    assert rows.n == keep.numel() and rows.total == B * S
    assert torch.equal(rows.idx.cpu().long(), keep) and torch.equal(rows.labels.cpu(), shift[keep])
    inv = rows.inv.cpu().long()
    assert torch.equal(inv[keep], torch.arange(keep.numel())) and int((inv < 0).sum()) == B * S - keep.numel()
    wide = rnd((B * S, H + 16), dtype, 12).cuda()
    x = wide[:, :H]                                                       # row stride H + 16
    y = K.rows_select(x, rows.idx, rows.n)
    assert torch.equal(y, x[keep.cuda()])
    dy = rnd((rows.n, H), dtype, 13).cuda()
    dx = K.rows_select(dy, rows.inv, rows.total)
    want = torch.zeros(B * S, H, dtype=dtype, device="cuda")
    want[keep.cuda()] = dy
    assert torch.equal(dx, want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [128258, 16384, 40000])
def test_argmax_softmax_long_rows(K, dtype, V, monkeypatch):
    """mm_argmax_softmax_split (the vocabulary in 4096-entry chunks over many workgroups, one 64-bit atomic max per chunk) picks what
    torch.argmax(torch.softmax(logits / T)) picks in the logits dtype and what the one-block-per-row kernel picks -- including ties
    between equal rounded probabilities (first index wins) and a padded row stride."""
    rows, ld = 5, (V + 63) // 64 * 64
    logits = rnd((rows, V), dtype, 91, 2.0)
    logits[1, 7] = logits[1].max() + 1.0                      # a clear winner early in the row
    logits[2, V - 3] = logits[2].max() + 1.0                  # ... and in the ragged tail of the last chunk
    logits[3, 5000] = logits[3, 9000] = logits[3].max() + 2.0   # an exact tie across two chunks: the first index wins
    buf = torch.full((rows, ld), float("nan"), dtype=dtype, device="cuda")
    buf[:, :V] = logits.cuda()
    for T_ in (0.1, 1.0):
        want = torch.argmax(torch.softmax(logits / T_, dim=-1), dim=-1)
        got = K.argmax_softmax(buf[:, :V], V, T_).cpu()
        monkeypatch.setenv("MM_ARGMAX_SPLIT", "0")
        one = K.argmax_softmax(buf[:, :V], V, T_).cpu()
        monkeypatch.setenv("MM_ARGMAX_SPLIT", "1")
        assert torch.equal(got, want) and torch.equal(got, one), (T_, got, want, one)
    assert int(got[1]) == 7 and int(got[2]) == V - 3 and int(got[3]) == 5000


