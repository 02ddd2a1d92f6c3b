"""The MXFP8 weight-only format of include/mm_hip.h (mm_quant_mxfp8) restated in torch, on any device: the reference the
quantiser kernels are compared with bit for bit, and the generator of the test matrices.

Per block of 32 consecutive k of a row: amax = max |w| (fp32); e = the smallest integer with amax * 2^-e <= 448 (e0 =
floor(log2 amax) - 8, plus one when amax * 2^-e0 > 448); scale byte = clamp(e + 127, 27, 254), 127 for a zero block; element =
e4m3fn(clamp(w * 2^-e, -448, 448)), round to nearest even (torch.float8_e4m3fn's conversion; it yields NaN above the range,
hence the clamp in front of it)."""
import torch

BLOCK = 32
E4M3_MAX = 448.0


def quant_ref(w, want_scaled=False):
    """w bf16 [N, K], K % 32 == 0 -> (q float8_e4m3fn [N, K], scale bytes uint8 [N, K // 32]); want_scaled: also w * 2^-e in fp32,
    the value in front of the clamp."""
    N, K = w.shape
    assert w.dtype == torch.bfloat16 and K % BLOCK == 0
    wf = w.float().view(N, K // BLOCK, BLOCK)
    amax = wf.abs().amax(dim=-1)
    _, ex = torch.frexp(amax)                                   # amax = m * 2^ex, m in [0.5, 1): floor(log2 amax) = ex - 1
    e0 = ex.to(torch.int32) - 1 - 8
    over = torch.ldexp(amax, -e0) > E4M3_MAX                    # exact: a power-of-two scaling of a bf16 value inside fp32's range
    e = e0 + over.to(torch.int32)
    byte = torch.where(amax == 0, torch.full_like(e, 127), (e + 127).clamp(27, 254))
    scaled = torch.ldexp(wf, (127 - byte).unsqueeze(-1).expand_as(wf))
    q = scaled.clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    # the sign of a zero survives the clamp and the conversion; an underflow keeps its sign as well
    if want_scaled:
        return q.view(N, K), byte.to(torch.uint8), scaled.view(N, K)
    return q.view(N, K), byte.to(torch.uint8)


def dequant_f32(q, byte):
    """element * 2^(byte - 127) in fp32 (exact)."""
    N, K = q.shape
    f = torch.ldexp(q.float().view(N, K // BLOCK, BLOCK), (byte.to(torch.int32) - 127).unsqueeze(-1).expand(N, K // BLOCK, BLOCK))
    return f.view(N, K)


def dequant_ref(q, byte):
    """-> W' bf16 [N, K]: the conversion rounds nothing (tests/test_w8_check_cpu.py)."""
    return dequant_f32(q, byte).to(torch.bfloat16)


def roundtrip_ref(w):
    return dequant_ref(*quant_ref(w))


def sample_matrix(N, K, seed, device="cpu"):
    """bf16 [N, K] that meets every branch of the format: per-block magnitudes spread over 2^+-20, all-zero blocks (with negative
    zeros), blocks whose amax * 2^-e0 sits just below, at and just above 448, tiny elements beside a large amax (e4m3 subnormals
    and underflow)."""
    g = torch.Generator().manual_seed(seed)
    nb = K // BLOCK
    w = torch.randn(N, nb, BLOCK, generator=g)
    w = w * torch.exp2(torch.randint(-20, 21, (N, nb, 1), generator=g).float())
    w = w * torch.exp2(-torch.randint(0, 16, (N, nb, BLOCK), generator=g).float() * (torch.rand(N, nb, BLOCK, generator=g) < 0.25))
    w = w.to(torch.bfloat16)
    flat = w.view(N * nb, BLOCK)
    kind = torch.arange(N * nb) % 7
    flat[kind == 0] = 0.0
    flat[kind == 0, ::3] = -0.0
    # amax mantissas around the 448 = 1.75 * 2^8 boundary: 1.7421875 (0x5F), 1.75 (0x60), 1.7578125 (0x61) times a power of two
    for k, mant in ((1, 1.7421875), (2, 1.75), (3, 1.7578125)):
        rows = (kind == k).nonzero().flatten()
        if rows.numel():
            scale = torch.exp2(torch.randint(-30, 31, (rows.numel(),), generator=g).float())
            blockv = flat[rows].float()
            blockv = blockv / blockv.abs().amax(dim=-1, keepdim=True).clamp_min(1e-30) * 0.9 * scale[:, None]
            blockv[:, 5] = -mant * scale
            flat[rows] = blockv.to(torch.bfloat16)
    return w.view(N, K).to(device)
