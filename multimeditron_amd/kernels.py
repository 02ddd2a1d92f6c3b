"""Tensor-level wrappers over the C ABI (include/mm_hip.h).  torch is used for device memory and the current
HIP stream only; every arithmetic step below is a libmmhip kernel.  No autograd here (see functional.py)."""
from __future__ import annotations

import ctypes
import math
import os
from typing import Optional

import torch

from . import _lib
from ._lib import (EPI_ACCUMULATE, EPI_BIAS, EPI_GELU_ERF, EPI_QUICK_GELU, EPI_RESIDUAL, GEMM_NN, GEMM_NT, GEMM_TN,
                   MM_BF16, MM_F32, call)

_DT = {torch.bfloat16: MM_BF16, torch.float32: MM_F32}


def dt(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"libmmhip supports bf16/f32 tensors, got {t.dtype}") from None


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.MMHipError("libmmhip kernels need device tensors (no CPU fallback)")
    return t.data_ptr()


def pad8(n: int) -> int:
    return (n + 7) // 8 * 8


# A/B switches of the environment (tools/step_ab.py, tools/decode_bench.py, the tests): name -> (default, what the other value selects).
# Read at call time: the tools and the tests flip them inside one process.
SWITCHES = {
    "MM_FUSED_GELU": ("1", "0: Linear + GELU as mm_gemm + mm_gelu_fwd (+ mm_add) instead of mm_gemm_act_fwd"),
    "MM_FUSED_SWIGLU": ("1", "0: mm_gemm + the separate SwiGLU kernels instead of mm_gemm_swiglu_fwd / _bwd"),
    "MM_FUSED_ROPE": ("1", "0: mm_gemm + mm_rope_apply instead of mm_gemm_rope_fwd"),
    "MM_DECODE_FUSED": ("1", "0: a decode step's norms and SwiGLU as separate launches"),
    "MM_DECODE_MERGE": ("launch", "fused: mm_attn_decode merges its slices itself (arrival counters) instead of a second launch"),
    "MM_ARGMAX_SPLIT": ("1", "0: mm_argmax_softmax on long rows too, instead of mm_argmax_softmax_split"),
}


def switch(name: str) -> str:
    return os.environ.get(name, SWITCHES[name][0])


def _on(name: str) -> bool:
    return os.environ.get(name, SWITCHES[name][0]) != "0"


def _sizes(symbol: str, *args, n: int = 1):
    """the int64_t* out-parameter(s) at the end of a size query: one value, or a tuple of n"""
    outs = [ctypes.c_int64(0) for _ in range(n)]
    call(symbol, *args, *[ctypes.byref(o) for o in outs])
    return outs[0].value if n == 1 else tuple(o.value for o in outs)


def _rows_out(M: int, N: int, like: torch.Tensor, ldc_pad: bool = False) -> torch.Tensor:
    """a new [M, N] output in like's dtype on its device; ldc_pad: a view of a buffer whose row stride is N rounded up to 64"""
    ld = (N + 63) // 64 * 64 if ldc_pad else N
    buf = torch.empty((M, ld), dtype=like.dtype, device=like.device)
    return buf[:, :N] if ld != N else buf


def fused_gelu_ok(dtype, rows: int) -> bool:
    """what mm_gemm_act_fwd (and its grouped form, per problem) takes: bf16 and more than 16 rows"""
    return dtype == torch.bfloat16 and rows > 16 and _on("MM_FUSED_GELU")


# ------------------------------------------------------------------------------------------------ GEMM
def gemm(layout: int, a: torch.Tensor, b: torch.Tensor, M: int, N: int, K: int, out: Optional[torch.Tensor] = None,
         bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, act: int = 0,
         accumulate: bool = False, ldc_pad: bool = False) -> torch.Tensor:
    """Raw GEMM on 2-D row-major tensors (strides taken from .stride(0)).  Returns C [M, N] (a view of a padded
    buffer when ldc_pad)."""
    assert a.dim() == 2 and b.dim() == 2 and a.stride(1) == 1 and b.stride(1) == 1
    if out is None:
        out = _rows_out(M, N, a, True) if ldc_pad else torch.empty((M, N), dtype=a.dtype, device=a.device)     # the common case without a call
    assert out.stride(1) == 1
    epi = act
    if bias is not None:
        epi |= EPI_BIAS
    if residual is not None:
        epi |= EPI_RESIDUAL
        assert residual.stride(-1) == 1
    if accumulate:
        epi |= EPI_ACCUMULATE
    call("mm_gemm", dt(a), layout, M, N, K, _p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), _p(bias),
         _p(residual), residual.stride(0) if residual is not None else 0, epi, _stream())
    return out


def linear_fwd(x2d, w, bias=None, residual=None, act=0, ldc_pad=False):
    """y[M,N] = x[M,K] @ w[N,K]^T (+bias)(act)(+residual)."""
    M, K = x2d.shape
    N = w.shape[0]
    return gemm(GEMM_NT, x2d, w, M, N, K, bias=bias, residual=residual, act=act, ldc_pad=ldc_pad)


def linear_act_fwd(x2d, w, bias, act, residual=None):
    """Training forward of Linear + GELU in one launch: -> (pre, y) with pre = bf16(x @ w^T + bias) kept for backward and
    y = act(pre) (+ residual).  Bit-identical to linear_fwd + gelu_fwd (+ add).  bf16 and M > 16 only: the caller falls back to the
    separate launches otherwise (this function returns None then)."""
    M, K = x2d.shape
    N = w.shape[0]
    if not fused_gelu_ok(x2d.dtype, M):
        return None
    assert x2d.stride(1) == 1 and w.stride(1) == 1
    pre = torch.empty((M, N), dtype=x2d.dtype, device=x2d.device)
    y = torch.empty((M, N), dtype=x2d.dtype, device=x2d.device)
    epi = act | (EPI_BIAS if bias is not None else 0) | (EPI_RESIDUAL if residual is not None else 0)
    call("mm_gemm_act_fwd", dt(x2d), M, N, K, _p(x2d), x2d.stride(0), _p(w), w.stride(0), _p(bias), _p(pre), pre.stride(0), _p(y),
         y.stride(0), _p(residual), residual.stride(0) if residual is not None else 0, epi, _stream())
    return pre, y


def linear_dgrad(dy2d, w, out=None):
    """dx[M,K] = dy[M,N] @ w[N,K]."""
    M = dy2d.shape[0]
    N, K = w.shape
    return gemm(GEMM_NN, dy2d, w, M, K, N, out=out)


def linear_wgrad(dy2d, x2d, out, accumulate):
    """dw[N,K] (+)= dy[M,N]^T @ x[M,K]."""
    M, N = dy2d.shape
    K = x2d.shape[1]
    return gemm(GEMM_TN, dy2d, x2d, N, K, M, out=out, accumulate=accumulate)


def gemm_swiglu_fwd(x2d, wgu, I):
    """(gu [M, 2I], act [M, I]) = fused gate|up GEMM + SwiGLU; None when the shape must take the two-launch form."""
    M, K = x2d.shape
    if x2d.dtype != torch.bfloat16 or (I % 128) or (K % 64) or M < 256 or not _on("MM_FUSED_SWIGLU"):
        return None
    gu = torch.empty((M, 2 * I), dtype=x2d.dtype, device=x2d.device)
    act = torch.empty((M, I), dtype=x2d.dtype, device=x2d.device)
    call("mm_gemm_swiglu_fwd", dt(x2d), M, I, K, _p(x2d), x2d.stride(0), _p(wgu), wgu.stride(0), _p(gu), gu.stride(0), _p(act),
         act.stride(0), _stream())
    return gu, act


def gemm_rope_fwd(x2d, w, bias, rope_cols, D, cos, sin):
    """qkv [M, N] = x @ w^T (+ bias) with RoPE on the first rope_cols columns, in one launch; None when the shape must take the
    two-launch form (mm_gemm + mm_rope_apply: same bits)."""
    M, K = x2d.shape
    N = w.shape[0]
    if (x2d.dtype != torch.bfloat16 or D != 128 or (N % 128) or (rope_cols % 128) or M < 256 or not _on("MM_FUSED_ROPE")
            or cos.dtype != torch.float32 or cos.shape[-1] != D // 2):
        return None
    out = torch.empty((M, N), dtype=x2d.dtype, device=x2d.device)
    call("mm_gemm_rope_fwd", dt(x2d), M, N, K, _p(x2d), x2d.stride(0), _p(w), w.stride(0), _p(bias), _p(out), out.stride(0), int(rope_cols),
         int(D), _p(cos), _p(sin), _stream())
    return out


# ---- decode-step fusions (M = batch <= 16 rows; see include/mm_hip.h) ----------------------------------------------------------
def decode_fits(M, K):
    """x (M rows of K bf16) must fit the weight-streaming kernel's LDS stage."""
    return K % 8 == 0 and M * K * 2 <= 143 * 1024        # csrc/mm_gemm.hip GEMV_X_LDS_MAX (160 KB minus the kernel's static reduction scratch)


def _cache_rows(kcache, vcache, D, pos):
    """a decode step's cache arguments: the pointers of cache[:, pos] ([B, Smax, Hkv, D], contiguous in the last two) and the batch stride"""
    assert kcache.stride(3) == 1 and kcache.stride(2) == D and vcache.stride(2) == D and kcache.stride(0) == vcache.stride(0)
    return _p(kcache[:, pos]), _p(vcache[:, pos]), kcache.stride(0)


def _weight_args(w, packed):
    """how a weight-streaming launch takes its matrix: (symbol suffix, arguments) of the bf16 matrix w, or of its MXFP8 copy"""
    return ("_w8", (_p(packed),)) if packed is not None else ("", (_p(w), w.stride(0)))


def decode_gateup_swiglu(x2d, wgu, I, norm_w=None, eps=0.0, out=None, packed=None):
    """act [M, I] = silu(x' Wg^T) * (x' Wu^T), x' = rmsnorm(x) * norm_w when norm_w is given.  packed: the MXFP8 copy of the fused
    [2I, K] gate|up matrix, read in place of wgu: the bits of the bf16 call on dequant_mxfp8(packed)."""
    M, K = x2d.shape
    act = _rows_out(M, I, x2d) if out is None else out
    sfx, wargs = _weight_args(wgu, packed)
    call("mm_decode_gateup_swiglu" + sfx, dt(x2d), M, I, K, _p(x2d), x2d.stride(0), *wargs, _p(act), act.stride(0), _p(norm_w), float(eps),
         _stream())
    return act


def decode_qkv_rope_append(x2d, w, bias, Hq, Hkv, D, cos, sin, kcache, vcache, pos, norm_w=None, eps=0.0, out=None, packed=None):
    """qkv [B, (Hq+2Hkv)*D] = x' @ w^T (+ bias) with RoPE on q / k and the append of roped k / v to cache[:, pos].  packed: the MXFP8
    copy of the fused q|k|v matrix, read in place of w."""
    M, K = x2d.shape
    cache = _cache_rows(kcache, vcache, D, pos)
    qkv = _rows_out(M, (Hq + 2 * Hkv) * D, x2d) if out is None else out
    sfx, wargs = _weight_args(w, packed)
    call("mm_decode_qkv_rope_append" + sfx, dt(x2d), M, Hq, Hkv, D, K, _p(x2d), x2d.stride(0), *wargs, _p(bias), _p(qkv), qkv.stride(0),
         _p(cos), _p(sin), *cache, _p(norm_w), float(eps), _stream())
    return qkv


def decode_linear(x2d, w, bias=None, residual=None, norm_w=None, eps=0.0, ldc_pad=False, out=None, packed=None, N=None):
    """c [M, N] = x' @ w^T (+ bias) (+ residual), x' = rmsnorm(x) * norm_w when norm_w is given; ldc_pad: row stride padded to 64.
    packed: the MXFP8 copy of w [N, K], read in place of w (N must be given then)."""
    M, K = x2d.shape
    N = w.shape[0] if packed is None else N
    c = _rows_out(M, N, x2d, ldc_pad) if out is None else out
    sfx, wargs = _weight_args(w, packed)
    call("mm_decode_linear" + sfx, dt(x2d), M, N, K, _p(x2d), x2d.stride(0), *wargs, _p(bias), _p(residual),
         residual.stride(0) if residual is not None else 0, _p(c), c.stride(0), _p(norm_w), float(eps), _stream())
    return c[:, :N] if c.shape[1] != N else c


# ---- weight-only MXFP8 copies for the decode step (include/mm_hip.h: e4m3 elements, one power-of-two scale per 32 k) ---------------
def mxfp8_bytes(N, K):
    n = _lib.lib().mm_mxfp8_bytes(int(N), int(K))
    if n < 0:
        raise _lib.MMHipError(f"mm_mxfp8_bytes({N}, {K}) failed: {n} (K must be a multiple of 32)")
    return n


def quant_mxfp8(w, out=None):
    """packed uint8 [mxfp8_bytes(N, K)] of a bf16 matrix w [N, K] (row stride w.stride(0)); the layout is the library's own."""
    assert w.dim() == 2 and w.stride(1) == 1
    if w.dtype != torch.bfloat16:
        raise TypeError(f"quant_mxfp8 takes a bf16 matrix, got {w.dtype}")
    N, Kd = w.shape
    if out is None:
        out = torch.empty((mxfp8_bytes(N, Kd),), dtype=torch.uint8, device=w.device)
    call("mm_quant_mxfp8", _p(w), w.stride(0), N, Kd, _p(out), _stream())
    return out


def dequant_mxfp8(packed, N, K, out=None):
    """The bf16 matrix W' [N, K] a packed buffer stands for (exact: e4m3 times a power of two is a bf16 number)."""
    if out is None:
        out = torch.empty((N, K), dtype=torch.bfloat16, device=packed.device)
    assert out.stride(1) == 1
    call("mm_dequant_mxfp8", _p(packed), N, K, _p(out), out.stride(0), _stream())
    return out


def decode_gateup_swiglu_w8(x2d, packed, I, norm_w=None, eps=0.0, out=None):
    return decode_gateup_swiglu(x2d, None, I, norm_w, eps, out, packed)


def decode_qkv_rope_append_w8(x2d, packed, bias, Hq, Hkv, D, cos, sin, kcache, vcache, pos, norm_w=None, eps=0.0, out=None):
    return decode_qkv_rope_append(x2d, None, bias, Hq, Hkv, D, cos, sin, kcache, vcache, pos, norm_w, eps, out, packed)


def decode_linear_w8(x2d, packed, N, bias=None, residual=None, norm_w=None, eps=0.0, ldc_pad=False, out=None):
    return decode_linear(x2d, None, bias, residual, norm_w, eps, ldc_pad, out, packed, N)


# ---- MXFP8 x MXFP8 GEMM for the prefill (include/mm_hip.h: mm_gemm_mx8, the block-scaled MFMA) -----------------------------------
def gemm_mx8_supported(M, N, K):
    """None, or why mm_gemm_mx8 refuses the shape (host only: no launch, no device)."""
    rc = _lib.lib().mm_gemm_mx8_supported(int(M), int(N), int(K))
    if rc == 0:
        return None
    if rc == _lib.ERR_UNSUPPORTED:
        return f"mm_gemm_mx8 takes K % 128 == 0 (K <= 2^20), got K = {K}"
    return f"mm_gemm_mx8 refuses M = {M}, N = {N}, K = {K} ({rc})"


def gemm_mx8(packedA, M, packedW, N, K, bias=None, residual=None, out=None):
    """c [M, N] (bf16) = A' @ W'^T (+ bias) (+ residual) from two quant_mxfp8 buffers (A' [M, K], W' [N, K] what dequant_mxfp8 returns);
    residual may be out.  fp32 accumulation, one rounding, the same bits on every call."""
    why = gemm_mx8_supported(M, N, K)
    if why is not None:
        raise _lib.MMHipError(why)
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=packedA.device)
    assert out.dtype == torch.bfloat16 and out.stride(1) == 1
    epi = 0
    if bias is not None:
        assert bias.dtype == torch.bfloat16
        epi |= EPI_BIAS
    if residual is not None:
        assert residual.dtype == torch.bfloat16 and residual.stride(-1) == 1
        epi |= EPI_RESIDUAL
    call("mm_gemm_mx8", int(M), int(N), int(K), _p(packedA), _p(packedW), _p(bias), _p(residual),
         residual.stride(0) if residual is not None else 0, _p(out), out.stride(0), epi, _stream())
    return out


def decode_fusions():
    return _on("MM_DECODE_FUSED")


def gemm_swiglu_bwd(dy2d, wd, gu, I):
    """dgu [M, 2I] from dy [M, H], down_proj weight [H, I] and the saved pre-activations; None -> two-launch form."""
    M, H = dy2d.shape
    if dy2d.dtype != torch.bfloat16 or (I % 4) or not _on("MM_FUSED_SWIGLU"):
        return None
    dgu = torch.empty_like(gu)
    call("mm_gemm_swiglu_bwd", dt(dy2d), M, I, H, _p(dy2d), dy2d.stride(0), _p(wd), wd.stride(0), _p(gu), gu.stride(0), _p(dgu),
         dgu.stride(0), _stream())
    return dgu


def colsum(x2d, out, accumulate):
    call("mm_colsum", dt(x2d), _p(x2d), x2d.shape[0], x2d.shape[1], x2d.stride(0), _p(out), int(accumulate), _stream())
    return out


# ------------------------------------------------------------------------------------------------ grouped launches
# `groups` equal-shaped problems in ONE launch (the MoE image modality's expert towers): per-problem operands are lists of 2-D
# tensors with equal strides; the pointers travel as host arrays (include/mm_hip.h, "grouped launches").
def _pa(ts):
    """host array of device pointers (None for an absent operand)"""
    if ts is None:
        return None
    return (ctypes.c_void_p * len(ts))(*[_p(t) for t in ts])


def _pat(ts, g):
    """the pointer of problem g's operand (None for an absent operand)"""
    return _p(ts[g]) if ts is not None else None


def _same_stride(ts):
    ld = ts[0].stride(0)
    assert all(t.dim() == 2 and t.stride(1) == 1 and t.stride(0) == ld and t.dtype == ts[0].dtype for t in ts)
    return ld


def _grouped_or_each(G, grouped, each):
    """grouped(): one launch for G problems; the problems the grouped kernels do not cover (MM_ERR_UNSUPPORTED) run each(g) one by one"""
    try:
        grouped()
    except _lib.MMHipError as err:
        if getattr(err, "code", None) != _lib.ERR_UNSUPPORTED:
            raise
        for g in range(G):
            each(g)


def gemm_batched(layout, As, Bs, M, N, K, outs, biases=None, residuals=None, act=0, accumulate=False):
    """mm_gemm on every (As[g], Bs[g]) -> outs[g] in one launch; problems the grouped kernels do not cover (those that fill the
    chip on their own: 256-wide tiles, M <= 16) are looped through mm_gemm -- same bits either way."""
    epi = act | (EPI_BIAS if biases is not None else 0) | (EPI_RESIDUAL if residuals is not None else 0) | (EPI_ACCUMULATE if accumulate else 0)
    lda, ldb, ldc = _same_stride(As), _same_stride(Bs), _same_stride(outs)
    ldr = _same_stride(residuals) if residuals is not None else 0
    _grouped_or_each(len(As),
                     lambda: call("mm_gemm_batched", dt(As[0]), layout, len(As), M, N, K, _pa(As), lda, _pa(Bs), ldb, _pa(outs), ldc, _pa(biases),
                                  _pa(residuals), ldr, epi, _stream()),
                     lambda g: call("mm_gemm", dt(As[g]), layout, M, N, K, _p(As[g]), lda, _p(Bs[g]), ldb, _p(outs[g]), ldc, _pat(biases, g),
                                    _pat(residuals, g), ldr, epi, _stream()))
    return outs


def _rows(t, groups):
    """the `groups` equal row blocks of an expert-major 2-D tensor"""
    R = t.shape[0] // groups
    return [t[g * R:(g + 1) * R] for g in range(groups)]


def linear_fwd_batched(x, ws, biases=None, residual=None, act=0):
    """x [G*R, K] expert-major, ws[g] [N, K] -> y [G*R, N]: y_g = x_g @ ws[g]^T (+ bias_g) (act) (+ residual_g)."""
    G = len(ws)
    R, Kd = x.shape[0] // G, x.shape[1]
    N = ws[0].shape[0]
    y = torch.empty((G * R, N), dtype=x.dtype, device=x.device)
    gemm_batched(GEMM_NT, _rows(x, G), ws, R, N, Kd, _rows(y, G), biases=biases, residuals=_rows(residual, G) if residual is not None else None,
                 act=act)
    return y


def linear_act_fwd_batched(x, ws, biases, act, residual=None):
    """linear_act_fwd on every expert's rows in one launch -> (pre, y) [G*R, N], or None where the separate launches must run."""
    G = len(ws)
    R, Kd = x.shape[0] // G, x.shape[1]
    N = ws[0].shape[0]
    if not fused_gelu_ok(x.dtype, R):
        return None
    pre = torch.empty((G * R, N), dtype=x.dtype, device=x.device)
    y = torch.empty((G * R, N), dtype=x.dtype, device=x.device)
    xs, pres, ys = _rows(x, G), _rows(pre, G), _rows(y, G)
    res = _rows(residual, G) if residual is not None else None
    epi = act | (EPI_BIAS if biases is not None else 0) | (EPI_RESIDUAL if residual is not None else 0)
    ldx, ldw = _same_stride(xs), _same_stride(ws)
    ldr = residual.stride(0) if residual is not None else 0
    _grouped_or_each(G,
                     lambda: call("mm_gemm_act_fwd_batched", dt(x), G, R, N, Kd, _pa(xs), ldx, _pa(ws), ldw, _pa(biases), _pa(pres), pre.stride(0),
                                  _pa(ys), y.stride(0), _pa(res), ldr, epi, _stream()),
                     lambda g: call("mm_gemm_act_fwd", dt(x), R, N, Kd, _p(xs[g]), ldx, _p(ws[g]), ldw, _pat(biases, g), _p(pres[g]), pre.stride(0),
                                    _p(ys[g]), y.stride(0), _pat(res, g), ldr, epi, _stream()))
    return pre, y


def linear_dgrad_batched(dy, ws):
    """dx [G*R, K] = dy_g [R, N] @ ws[g] [N, K] per expert."""
    G = len(ws)
    R = dy.shape[0] // G
    N, Kd = ws[0].shape
    dx = torch.empty((G * R, Kd), dtype=dy.dtype, device=dy.device)
    gemm_batched(GEMM_NN, _rows(dy, G), ws, R, Kd, N, _rows(dx, G))
    return dx


def linear_wgrad_batched(dy, x, outs, accumulate):
    """outs[g] [N, K] (+)= dy_g^T @ x_g per expert."""
    G = len(outs)
    R, N = dy.shape[0] // G, dy.shape[1]
    gemm_batched(GEMM_TN, _rows(dy, G), _rows(x, G), N, x.shape[1], R, outs, accumulate=accumulate)


def colsum_batched(x, outs, accumulate):
    """outs[g] [N] (+)= the column sums of expert g's rows of x [G*R, N]."""
    G = len(outs)
    xs = _rows(x, G)
    call("mm_colsum_batched", dt(x), _pa(xs), G, xs[0].shape[0], x.shape[1], x.stride(0), _pa(outs), int(accumulate), _stream())


def layernorm_fwd_batched(x2d, ws, bs, eps):
    G = len(ws)
    M, H = x2d.shape
    y = torch.empty_like(x2d)
    mean = torch.empty(M, dtype=torch.float32, device=x2d.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x2d.device)
    call("mm_layernorm_fwd_batched", dt(x2d), _p(x2d), _pa(ws), _pa(bs), G, M // G, H, float(eps), _p(y), _p(mean), _p(rstd), _stream())
    return y, mean, rstd


def layernorm_bwd_batched(dy2d, x2d, ws, mean, rstd, dres=None):
    """-> (dx, dw partials, db partials); expert g's partial blocks are rows [g*nb, (g+1)*nb), nb = norm_bwd_blocks(R)."""
    G = len(ws)
    M, H = x2d.shape
    R = M // G
    dx = torch.empty_like(x2d)
    nb = norm_bwd_blocks(R)
    dwp = torch.empty((G * nb, H), dtype=torch.float32, device=x2d.device)
    dbp = torch.empty((G * nb, H), dtype=torch.float32, device=x2d.device)
    call("mm_layernorm_bwd_batched", dt(x2d), _p(dy2d), _p(x2d), _pa(ws), G, _p(mean), _p(rstd), R, H, _p(dx), _p(dwp), _p(dbp), _p(dres),
         _stream())
    return dx, dwp, dbp


def reduce_partials2_batched(partial0, partial1, outs0, outs1, accumulate0, accumulate1):
    G = len(outs0)
    assert partial0.shape == partial1.shape and partial0.shape[0] % G == 0
    call("mm_reduce_partials2_batched", dt(outs0[0]), _p(partial0), _p(partial1), G, partial0.shape[0] // G, partial0.shape[1], _pa(outs0),
         _pa(outs1), int(accumulate0), int(accumulate1), _stream())


# ------------------------------------------------------------------------------------------------ splice
def splice_build_map(batch_idx, token_range, S, T):
    m = torch.empty(T, dtype=torch.int32, device=batch_idx.device if batch_idx is not None else "cuda")
    n = 0 if batch_idx is None else batch_idx.numel()
    call("mm_splice_build_map", _p(batch_idx) if n else None, _p(token_range) if n else None, n, S, T, _p(m), _stream())
    return m


_oor_state = {}          # device index -> [device flag, pinned host copy, event of the last copy]


def embed_check_ids(ids, vocab, block=False):
    """nn.Embedding's range check without a stall: a tiny kernel raises a sticky device flag for ids outside [0, vocab); the
    flag travels to pinned memory behind it, and the host looks at the copy of the PREVIOUS call (complete by then), or waits for
    this one with block=True.  Raises IndexError like torch (reference model.py:433: every id of the batch is embedded)."""
    dev = ids.device.index or 0
    st = _oor_state.get(dev)
    if st is None:
        st = _oor_state[dev] = [torch.zeros(1, dtype=torch.int32, device=ids.device), torch.zeros(1, dtype=torch.int32).pin_memory(), None]
    _embed_raise_if_flagged(st, wait=False)
    call("mm_embed_check_ids", _p(ids), ids.numel(), int(vocab), _p(st[0]), _stream())
    st[1].copy_(st[0], non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    st[2] = ev
    if block:
        _embed_raise_if_flagged(st, wait=True)


def embed_check_pending():
    """Wait for the outstanding id checks of every device and raise if one failed (called where the host synchronises anyway)."""
    for st in _oor_state.values():
        _embed_raise_if_flagged(st, wait=True)


def _embed_raise_if_flagged(st, wait):
    ev = st[2]
    if ev is None:
        return
    if wait:
        ev.synchronize()
    elif not ev.query():
        return
    st[2] = None
    if int(st[1][0]) != 0:
        st[0].zero_()
        st[1].zero_()
        raise IndexError("index out of range in self")


def embed_splice_fwd(emb, ids, proj, src_map):
    embed_check_ids(ids, emb.shape[0])
    T = ids.numel()
    H = emb.shape[1]
    out = torch.empty((T, H), dtype=emb.dtype, device=emb.device)
    call("mm_embed_splice_fwd", dt(emb), _p(emb), emb.shape[0], H, _p(ids), _p(proj), _p(src_map) if proj is not None else None, T,
         _p(out), _stream())
    return out


def embed_sort(ids, src_map, vocab, H):
    """Stable token order by id for the embedding gradient -> (order, skey) int32 (padded, see mm_embed_sort_sizes)."""
    T = ids.numel()
    n_order, _ = _sizes("mm_embed_sort_sizes", T, H, n=2)
    order = torch.empty(n_order, dtype=torch.int32, device=ids.device)
    skey = torch.empty(n_order, dtype=torch.int32, device=ids.device)
    ws = torch.empty(max(T, 1), dtype=torch.int32, device=ids.device)
    call("mm_embed_sort", _p(ids), _p(src_map), T, vocab, _p(ws), _p(order), _p(skey), _stream())
    return order, skey


def embed_splice_bwd(dE, ids, src_map, batch_idx, token_range, S, dproj, demb, order=None, skey=None, accumulate=False):
    T, H = dE.shape
    n = 0 if batch_idx is None else batch_idx.numel()
    scratch = None
    if demb is not None:
        scratch = torch.empty(((T + 31) // 32) * 2 * H, dtype=torch.float32, device=dE.device)
    call("mm_embed_splice_bwd", dt(dE), _p(dE), H, _p(ids), _p(src_map), T, _p(batch_idx) if n else None,
         _p(token_range) if n else None, n, S, _p(dproj), _p(demb), demb.shape[0] if demb is not None else 0, _p(order), _p(skey),
         _p(scratch), int(accumulate), _stream())


# ------------------------------------------------------------------------------------------------ ViT glue
def patchify(pixels, ps, kpad, dtype):
    n, c, h, w = pixels.shape
    assert c == 3 and pixels.dtype == torch.float32 and pixels.is_contiguous()
    P = (h // ps) * (w // ps)
    out = torch.empty((n * P, kpad), dtype=dtype, device=pixels.device)
    call("mm_patchify", _DT[dtype], _p(pixels), n, h, w, ps, kpad, _p(out), _stream())
    return out


def vit_embed_fwd(patch_out, cls, pos, n, P):
    D = cls.numel()
    x = torch.empty((n, P + 1, D), dtype=patch_out.dtype, device=patch_out.device)
    call("mm_vit_embed_fwd", dt(patch_out), _p(patch_out), _p(cls), _p(pos), n, P, D, _p(x), _stream())
    return x


def vit_embed_bwd(dx, dcls, dpos, accumulate, want_dpatch=True):
    n, T, D = dx.shape
    P = T - 1
    dpatch = torch.empty((n * P, D), dtype=dx.dtype, device=dx.device) if want_dpatch else None
    call("mm_vit_embed_bwd", dt(dx), _p(dx), n, P, D, _p(dpatch), _p(dcls), _p(dpos), int(accumulate), _stream())
    return dpatch


def bcast_add(x, b):
    """y[n, ...] = x[n, ...] + b[...] (b broadcast over the leading axis)."""
    y = torch.empty_like(x)
    call("mm_bcast_add", dt(x), _p(x), _p(b), x.shape[0], b.numel(), _p(y), _stream())
    return y


def head_pad(x2d, nheads, d, dpad, inverse=False):
    """[rows, nheads*d] -> [rows, nheads*dpad] (zero-padded heads), or back with inverse=True."""
    rows = x2d.shape[0]
    assert x2d.is_contiguous() and x2d.shape[1] == nheads * (dpad if inverse else d)
    out = torch.empty((rows, nheads * (d if inverse else dpad)), dtype=x2d.dtype, device=x2d.device)
    call("mm_head_pad", dt(x2d), _p(x2d), rows, nheads, d, dpad, _p(out), int(inverse), _stream())
    return out


def drop_cls_fwd(x):
    n, T, D = x.shape
    out = torch.empty((n, T - 1, D), dtype=x.dtype, device=x.device)
    call("mm_drop_cls_fwd", dt(x), _p(x), n, T - 1, D, _p(out), _stream())
    return out


def drop_cls_bwd(dy):
    n, P, D = dy.shape
    out = torch.empty((n, P + 1, D), dtype=dy.dtype, device=dy.device)
    call("mm_drop_cls_bwd", dt(dy), _p(dy), n, P, D, _p(out), _stream())
    return out


def rows_select(src2d, row_map, n_dst):
    """dst[r] = src2d[row_map[r]] (zeros where row_map[r] < 0); row_map int32 on the device, n_dst known to the host."""
    D = src2d.shape[1]
    assert row_map.dtype == torch.int32 and row_map.is_contiguous() and row_map.numel() >= n_dst and src2d.stride(1) == 1
    out = torch.empty((n_dst, D), dtype=src2d.dtype, device=src2d.device)
    call("mm_rows_select", dt(src2d), _p(src2d), src2d.stride(0), _p(row_map), src2d.shape[0], n_dst, D, _p(out), D, _stream())
    return out


# ------------------------------------------------------------------------------------------------ norms
def rmsnorm_fwd(x2d, w, eps):
    M, H = x2d.shape
    y = torch.empty_like(x2d)
    rstd = torch.empty(M, dtype=torch.float32, device=x2d.device)
    call("mm_rmsnorm_fwd", dt(x2d), _p(x2d), _p(w), M, H, float(eps), _p(y), _p(rstd), _stream())
    return y, rstd


def norm_bwd_blocks(M):
    return _lib.lib().mm_norm_bwd_blocks(M)


def rmsnorm_bwd(dy2d, x2d, w, rstd, dres=None):
    M, H = x2d.shape
    dx = torch.empty_like(x2d)
    dwp = torch.empty((norm_bwd_blocks(M), H), dtype=torch.float32, device=x2d.device)
    call("mm_rmsnorm_bwd", dt(x2d), _p(dy2d), _p(x2d), _p(w), _p(rstd), M, H, _p(dx), _p(dwp), _p(dres), _stream())
    return dx, dwp


def layernorm_fwd(x2d, w, b, eps):
    M, H = x2d.shape
    y = torch.empty_like(x2d)
    mean = torch.empty(M, dtype=torch.float32, device=x2d.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x2d.device)
    call("mm_layernorm_fwd", dt(x2d), _p(x2d), _p(w), _p(b), M, H, float(eps), _p(y), _p(mean), _p(rstd), _stream())
    return y, mean, rstd


def layernorm_bwd(dy2d, x2d, w, mean, rstd, dres=None):
    M, H = x2d.shape
    dx = torch.empty_like(x2d)
    nb = norm_bwd_blocks(M)
    dwp = torch.empty((nb, H), dtype=torch.float32, device=x2d.device)
    dbp = torch.empty((nb, H), dtype=torch.float32, device=x2d.device)
    call("mm_layernorm_bwd", dt(x2d), _p(dy2d), _p(x2d), _p(w), _p(mean), _p(rstd), M, H, _p(dx), _p(dwp), _p(dbp), _p(dres), _stream())
    return dx, dwp, dbp


def reduce_partials2(partial0, partial1, out0, out1, accumulate0, accumulate1):
    assert partial0.shape == partial1.shape and out0.dtype == out1.dtype
    call("mm_reduce_partials2", dt(out0), _p(partial0), _p(partial1), partial0.shape[0], partial0.shape[1], _p(out0), _p(out1), int(accumulate0),
         int(accumulate1), _stream())


def reduce_partials(partial, out, accumulate):
    call("mm_reduce_partials", dt(out), _p(partial), partial.shape[0], partial.shape[1], _p(out), int(accumulate), _stream())
    return out


# ------------------------------------------------------------------------------------------------ rope
def rope_table(position_ids, inv_freq, round_bf16):
    T = position_ids.numel()
    half = inv_freq.numel()
    cos = torch.empty((T, half), dtype=torch.float32, device=position_ids.device)
    sin = torch.empty_like(cos)
    call("mm_rope_table", _p(position_ids), _p(inv_freq), T, half, int(round_bf16), _p(cos), _p(sin), _stream())
    return cos, sin


def rope_apply_(x, T, nheads, D, ld, cos, sin, inverse=False):
    """in place on x (any tensor whose storage at data_ptr is [T, nheads, D] with row stride ld)."""
    call("mm_rope_apply", dt(x), _p(x), T, nheads, D, ld, _p(cos), _p(sin), int(inverse), _stream())
    return x


def rope_append_(qkv, B, Hq, Hkv, D, cos, sin, kcache, vcache, pos):
    """decode step: RoPE q/k in place + write roped k and v to cache[:, pos] ([B, Smax, Hkv, D] contiguous in the last two)."""
    call("mm_rope_append", dt(qkv), _p(qkv), B, Hq, Hkv, D, qkv.stride(0), _p(cos), _p(sin), *_cache_rows(kcache, vcache, D, pos), _stream())
    return qkv


def qk_norm_rope_fwd(qkv, T, Hq, Hkv, D, w_q, w_k, eps, cos, sin, out=None, want_rstd=True):
    """Qwen3: per-head RMSNorm (w_q / w_k) + RoPE of the q|k heads of qkv [T, >= (Hq+Hkv)*D] (row stride qkv.stride(0)).
    out: None -> a new [T, (Hq+Hkv)*D] buffer; out is qkv -> in place.  -> (qk, rstd [T, Hq+Hkv] f32 or None)."""
    assert qkv.stride(-1) == 1 and w_q.is_contiguous() and w_k.is_contiguous()
    if out is None:
        out = torch.empty((T, (Hq + Hkv) * D), dtype=qkv.dtype, device=qkv.device)
    rstd = torch.empty((T, Hq + Hkv), dtype=torch.float32, device=qkv.device) if want_rstd else None
    call("mm_qk_norm_rope_fwd", dt(qkv), _p(qkv), qkv.stride(0), T, Hq, Hkv, D, _p(w_q), _p(w_k), float(eps), _p(cos), _p(sin), _p(out),
         out.stride(0), _p(rstd), _stream())
    return out, rstd


def qk_norm_bwd_blocks(T):
    return _lib.lib().mm_qk_norm_bwd_blocks(T)


def qk_norm_rope_bwd(dqk, qkv, T, Hq, Hkv, D, w_q, w_k, rstd, cos, sin, dqkv, want_dw=True):
    """Writes d(raw q|k) into the q|k columns of dqkv (nothing else).  -> (dwq_partial, dwk_partial) [nblk, D] f32, or (None, None)."""
    assert dqk.stride(-1) == 1 and qkv.stride(-1) == 1 and dqkv.stride(-1) == 1 and rstd.is_contiguous()
    dwq = dwk = None
    if want_dw:
        nb = qk_norm_bwd_blocks(T)
        dwq = torch.empty((nb, D), dtype=torch.float32, device=qkv.device)
        dwk = torch.empty((nb, D), dtype=torch.float32, device=qkv.device)
    call("mm_qk_norm_rope_bwd", dt(qkv), _p(dqk), dqk.stride(0), _p(qkv), qkv.stride(0), T, Hq, Hkv, D, _p(w_q), _p(w_k), _p(rstd), _p(cos),
         _p(sin), _p(dqkv), dqkv.stride(0), _p(dwq), _p(dwk), _stream())
    return dwq, dwk


def qk_norm_rope_append_(qkv, B, Hq, Hkv, D, w_q, w_k, eps, cos, sin, kcache, vcache, pos):
    """decode step (Qwen3): per-head norm + RoPE of q/k in place + write the normed, roped k and v to cache[:, pos]."""
    call("mm_qk_norm_rope_append", dt(qkv), _p(qkv), B, Hq, Hkv, D, qkv.stride(0), _p(w_q), _p(w_k), float(eps), _p(cos), _p(sin),
         *_cache_rows(kcache, vcache, D, pos), _stream())
    return qkv


# ------------------------------------------------------------------------------------------------ attention
def _strides3(t):  # t: [B, S, H, D] view
    assert t.dim() == 4 and t.stride(3) == 1
    return t.stride(0), t.stride(1), t.stride(2)


def attn_fwd(q, k, v, key_mask, causal, scale):
    """q [B,Sq,Hq,D], k/v [B,Skv,Hkv,D] (strided views ok) -> out [B,Sq,Hq,D] contiguous, lse [B,Hq,Sq] f32."""
    B, Sq, Hq, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    out = torch.empty((B, Sq, Hq, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, Hq, Sq), dtype=torch.float32, device=q.device)
    call("mm_attn_fwd", dt(q), _p(q), _p(k), _p(v), B, Sq, Skv, Hq, Hkv, D, *_strides3(q), *_strides3(k), *_strides3(v),
         _p(key_mask), int(causal), float(scale), _p(out), _p(lse), _stream())
    return out, lse


def attn_bwd(q, k, v, out, dout, lse, key_mask, causal, scale, dq, dk, dv):
    """dq/dk/dv: preallocated views with the SAME strides as q/k/v."""
    B, Sq, Hq, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    assert _strides3(dq) == _strides3(q) and _strides3(dk) == _strides3(k) and _strides3(dv) == _strides3(v)
    assert dout.is_contiguous() and out.is_contiguous()
    delta = torch.empty((B, Hq, Sq), dtype=torch.float32, device=q.device)
    call("mm_attn_bwd", dt(q), _p(q), _p(k), _p(v), _p(out), _p(dout), _p(lse), B, Sq, Skv, Hq, Hkv, D, *_strides3(q),
         *_strides3(k), *_strides3(v), _p(key_mask), int(causal), float(scale), _p(dq), _p(dk), _p(dv), _p(delta), _stream())


def _decode_ws(q, ns):
    """(workspace of ns partial (out, max, sum) records per query row and head, out [rows, Hq, D]) of a decode-attention launch on q"""
    rows, Hq, D = q.shape
    return (torch.empty(rows * Hq * ns * (D + 2), dtype=torch.float32, device=q.device),
            torch.empty((rows, Hq, D), dtype=q.dtype, device=q.device))


def attn_decode_supported(q_dtype, Hq, Hkv, D):
    return q_dtype == torch.bfloat16 and D in (64, 128) and Hq % Hkv == 0 and (Hq // Hkv) in (1, 2, 4, 7, 8)


_decode_sync = {}


def attn_decode(q, k, v, key_mask, scale):
    """One query token per sequence over a KV cache: q [B,Hq,D] (strided view ok), k/v [B,Skv,Hkv,D] -> out [B,Hq,D]."""
    B, Hq, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    assert q.stride(2) == 1 and k.stride(3) == 1 and v.stride(3) == 1
    ns = _lib.lib().mm_attn_decode_splits(B, Hkv, Skv)
    ws, out = _decode_ws(q, ns)
    # sync=None: the slices are merged by a second (tiny) launch.  The single-launch form (sync = arrival counters [B * Hkv]; the
    # slice that arrives last merges) is correct but SLOWER on MI355X in every protocol tried: __threadfence() per thread (round 2:
    # 8.2 vs 5.2 ms/token), one agent-scope release per workgroup (round 3: the partial kernel went from 18 to 75 us -- buffer_wbl2
    # with an L2 full of dirty lines), write-through record stores + one acquire by the last arriver (33 us against 18 + 8 for the
    # two launches: the merging workgroup starts only when the last slice is done and reads records that come from beyond L2).
    # MM_DECODE_MERGE=fused selects it.
    sync = None
    if switch("MM_DECODE_MERGE") == "fused":
        sync = _decode_sync.get(q.device)
        if sync is None or sync.numel() < B * Hkv:
            sync = _decode_sync[q.device] = torch.zeros(max(64, B * Hkv), dtype=torch.int32, device=q.device)
    call("mm_attn_decode", dt(q), _p(q), _p(k), _p(v), B, Skv, Hq, Hkv, D, q.stride(0), q.stride(1), k.stride(0), k.stride(1),
         k.stride(2), v.stride(0), v.stride(1), v.stride(2), _p(key_mask), float(scale), _p(out), _p(ws), ns, _p(sync), _stream())
    return out


def attn_decode_shared_supported(q_dtype, Hq, Hkv, D):
    """Shapes mm_attn_decode_shared takes: bf16, head_dim 128, 1, 2 or 4 query heads per key/value head (16 / G samples share a
    16-column MFMA tile)."""
    return q_dtype == torch.bfloat16 and D == 128 and Hq % Hkv == 0 and (Hq // Hkv) in (1, 2, 4)


def attn_decode_shared(q, kp, vp, ks, vs, n, key_mask, scale, anc=None, nsplit=None):
    """One query token for each of the n samples of B prompts: q [B*n,Hq,D] (strided view ok; row b*n + j is sample j of prompt b)
    over prompt b's prefix kp/vp [B,Sp,Hkv,D] followed by the row's own suffix ks/vs [B*n,Ss,Hkv,D] -> out [B*n,Hq,D].  key_mask
    [B,Sp] or None covers the prefix; suffix keys are always visible.  The bits of attn_decode on the materialised concatenation
    (mm_attn_decode_shared).  With anc (int32 [>= Ss, >= B*n], last stride 1) suffix key t of row r is read from physical suffix row
    anc[t, r]: the bits of the call without it on the gathered suffix (mm_attn_decode_beam; attn_decode_beam below)."""
    R, Hq, D = q.shape
    B, Sp, Hkv = kp.shape[0], kp.shape[1], kp.shape[2]
    Ss = ks.shape[1]
    assert R == B * n and ks.shape[0] == R and vs.shape[0] == R and vp.shape[:3] == kp.shape[:3] and vs.shape[1] == Ss
    assert q.stride(2) == 1 and kp.stride(3) == 1 and vp.stride(3) == 1 and ks.stride(3) == 1 and vs.stride(3) == 1
    assert key_mask is None or (tuple(key_mask.shape) == (B, Sp) and key_mask.is_contiguous())
    assert anc is None or (anc.dtype == torch.int32 and anc.dim() == 2 and anc.shape[0] >= Ss and anc.shape[1] >= R and anc.stride(1) == 1)
    ns = _lib.lib().mm_attn_decode_shared_splits(B, n, Hkv, Sp + Ss) if nsplit is None else int(nsplit)
    ws, out = _decode_ws(q, ns)
    table = () if anc is None else (_p(anc), anc.stride(0))
    call("mm_attn_decode_shared" if anc is None else "mm_attn_decode_beam", dt(q), _p(q), _p(kp), _p(vp), _p(ks), _p(vs), B, n, Sp, Ss,
         Hq, Hkv, D, q.stride(0), q.stride(1), *_strides3(kp), *_strides3(vp), *_strides3(ks), *_strides3(vs), _p(key_mask), float(scale),
         _p(out), _p(ws), ns, *table, _stream())
    return out


def attn_decode_beam(q, kp, vp, ks, vs, n, key_mask, scale, anc, nsplit=None):
    """attn_decode_shared through the ancestor table anc, which this name requires (mm_attn_decode_beam)."""
    assert anc is not None
    return attn_decode_shared(q, kp, vp, ks, vs, n, key_mask, scale, anc, nsplit)


# ---- beam search (include/mm_hip.h: mm_beam_step) ----
BEAM_EARLY_STOPPING = {False: 0, True: 1, "never": 2}
BEAM_FIELDS = (("score", torch.float32), ("parent", torch.int32), ("tok", torch.int32), ("anc", torch.int32), ("fscore", torch.float32),
               ("flen", torch.int32), ("fseqno", torch.int32), ("fseq", torch.int32), ("open", torch.int32), ("fcount", torch.int32),
               ("done", torch.int32))


class BeamState:
    """The device state of one beam search of B prompts x n beams over at most T tokens: one buffer in the library's layout
    (mm_beam_state_layout) with a tensor view of every field, and the workspace of a step over V logits."""

    def __init__(self, B, n, T, V, device):
        nb = _sizes("mm_beam_state_bytes", int(B), int(n), int(T))
        wb = _sizes("mm_beam_ws_bytes", int(B), int(n), int(V))
        off = (ctypes.c_int64 * len(BEAM_FIELDS))()
        call("mm_beam_state_layout", int(B), int(n), int(T), off)
        self.B, self.n, self.T, self.V = int(B), int(n), int(T), int(V)
        self.buf = torch.zeros(nb, dtype=torch.uint8, device=device)
        self.ws = torch.empty((wb + 15) // 16 * 2, dtype=torch.int64, device=device)
        self.next_ids = torch.empty(B * n, dtype=torch.int64, device=device)
        R = B * n
        shapes = {"tok": (T, R), "anc": (2, T, R), "fseq": (R, T), "open": (B,), "fcount": (B,), "done": (1,)}
        for (name, dtype), o in zip(BEAM_FIELDS, off):
            shape = shapes.get(name, (R,))
            numel = math.prod(shape)
            setattr(self, name, self.buf[o:o + 4 * numel].view(dtype).view(shape))

    def table(self, step):
        """the ancestor table [T, R] of the decode step that produces the logits of `step` (mm_beam_step(step - 1) wrote it)"""
        return self.anc[step & 1]


def beam_step(logits2d, st: BeamState, step, eos, length_penalty=1.0, early_stopping=False):
    """rules a-g of mm_beam_step on logits [B (step 0) or B*n, >= V]; returns st.next_ids (the next embedding lookup)."""
    assert logits2d.stride(-1) == 1 and logits2d.shape[0] == (st.B if step == 0 else st.B * st.n)
    call("mm_beam_step", dt(logits2d), _p(logits2d), st.B, st.n, st.V, logits2d.stride(0), int(step), st.T, int(eos), float(length_penalty),
         BEAM_EARLY_STOPPING[early_stopping], _p(st.buf), st.buf.numel(), _p(st.ws), st.ws.numel() * 8, _p(st.next_ids), _stream())
    return st.next_ids


def beam_finish(st: BeamState, num_return, eos):
    """-> (ids int64 [B*num_return, T] eos-filled, scores f32 [B*num_return], lens i32 [B*num_return]) on the device."""
    rows = st.B * int(num_return)
    ids = torch.empty((rows, st.T), dtype=torch.int64, device=st.buf.device)
    scores = torch.empty(rows, dtype=torch.float32, device=st.buf.device)
    lens = torch.empty(rows, dtype=torch.int32, device=st.buf.device)
    call("mm_beam_finish", _p(st.buf), st.buf.numel(), st.B, st.n, st.T, int(num_return), int(eos), _p(ids), _p(scores), _p(lens), _stream())
    return ids, scores, lens


# ---- MXFP8 KV cache (include/mm_hip.h: e4m3 elements, one power-of-two scale per 32 d of a head; the buffer layout is the library's) ----
def kv8_bytes(B, Smax, Hkv, D):
    n = _lib.lib().mm_kv8_bytes(int(B), int(Smax), int(Hkv), int(D))
    if n < 0:
        raise _lib.MMHipError(f"mm_kv8_bytes({B}, {Smax}, {Hkv}, {D}) failed: {n} (head_dim must be 128)")
    return n


def kv8_append(k, v, cache, Smax, pos):
    """Quantise the bf16 rows k / v [B, S, Hkv, D] (strided views ok, head stride D) into positions pos .. pos + S - 1 of a cache buffer
    (uint8 [kv8_bytes(B, Smax, Hkv, D)])."""
    B, S, Hkv, D = k.shape
    assert v.shape == k.shape and k.stride(3) == 1 and v.stride(3) == 1 and k.stride(2) == D and v.stride(2) == D
    call("mm_kv8_append", dt(k), _p(k), _p(v), B, S, Hkv, D, k.stride(0), k.stride(1), v.stride(0), v.stride(1), _p(cache), Smax, pos,
         _stream())
    return cache


def kv8_dequant(cache, B, Smax, Hkv, D, pos=0, S=None):
    """The bf16 rows (k, v) [B, S, Hkv, D] the buffer stands for at positions pos .. pos + S - 1 (exact)."""
    S = Smax - pos if S is None else S
    k = torch.empty((B, S, Hkv, D), dtype=torch.bfloat16, device=cache.device)
    v = torch.empty_like(k)
    call("mm_kv8_dequant", _p(cache), B, Smax, Hkv, D, pos, S, _p(k), _p(v), k.stride(0), k.stride(1), _stream())
    return k, v


def attn_decode_kv8(q, cache, Skv, Smax, Hkv, key_mask, scale):
    """attn_decode over the first Skv positions of an MXFP8 cache buffer: q [B,Hq,D] (strided view ok) -> out [B,Hq,D].  The bits of
    attn_decode on kv8_dequant's rows whenever the slices coincide (mm_attn_decode_kv8)."""
    B, Hq, D = q.shape
    assert q.stride(2) == 1
    ns = _lib.lib().mm_attn_decode_splits(B, Hkv, Skv)
    ws, out = _decode_ws(q, ns)
    call("mm_attn_decode_kv8", dt(q), _p(q), _p(cache), B, Skv, Smax, Hq, Hkv, D, q.stride(0), q.stride(1), _p(key_mask), float(scale),
         _p(out), _p(ws), ns, _stream())
    return out


# ------------------------------------------------------------------------------------------------ small cross-attention + dropout
def xattn_supported(dtype, Nkv, D):
    """Shapes mm_xattn_* takes: up to 1024 keys (a query's whole score row lives in a wave's registers: 64 MFMA tiles; above 512 keys
    the kernel trades speed for it -- it spills -- which is fine at a cross-attention's size); bf16 head widths that are multiples of
    8 up to 512, any fp32 width whose score / query rows fit the wave-per-row kernel's LDS."""
    if Nkv > 1024:
        return False
    if dtype == torch.bfloat16:
        return D % 8 == 0 and D <= 512
    return dtype == torch.float32 and (2 * Nkv + 2 * D) * 4 <= 60000


def xattn_fwd(q, k, v, scale, drop_p=0.0, seed=0, offset=0):
    """q [n,Nq,H,D], k/v [n,Nkv,H,D] (strided views ok) -> out [n,Nq,H,D] contiguous, lse [n,H,Nq] f32; attention-probability
    dropout with probability drop_p from the Philox stream (seed, offset) (see include/mm_hip.h)."""
    n, Nq, H, D = q.shape
    Nkv = k.shape[1]
    out = torch.empty((n, Nq, H, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((n, H, Nq), dtype=torch.float32, device=q.device)
    call("mm_xattn_fwd", dt(q), _p(q), _p(k), _p(v), n, Nq, Nkv, H, D, *_strides3(q), *_strides3(k), *_strides3(v), float(scale),
         float(drop_p), int(seed), int(offset), _p(out), _p(lse), _stream())
    return out, lse


def xattn_bwd(q, k, v, out, dout, lse, scale, drop_p, seed, offset, dq, dk, dv):
    """dq/dk/dv: preallocated views with the SAME strides as q/k/v.  Deterministic (no atomics)."""
    n, Nq, H, D = q.shape
    Nkv = k.shape[1]
    assert _strides3(dq) == _strides3(q) and _strides3(dk) == _strides3(k) and _strides3(dv) == _strides3(v)
    assert dout.is_contiguous() and out.is_contiguous()
    nb = _sizes("mm_xattn_ws_bytes", dt(q), n, Nq, Nkv, H)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=q.device)
    call("mm_xattn_bwd", dt(q), _p(q), _p(k), _p(v), _p(out), _p(dout), _p(lse), n, Nq, Nkv, H, D, *_strides3(q), *_strides3(k),
         *_strides3(v), float(scale), float(drop_p), int(seed), int(offset), _p(dq), _p(dk), _p(dv), _p(ws), nb, _stream())


def dropout(x, p, seed, offset):
    """y = x * keep / (1 - p) with keep from the Philox stream (seed, offset); its own adjoint (apply it to dy)."""
    x = x.contiguous()
    y = torch.empty_like(x)
    call("mm_dropout", dt(x), _p(x), x.numel(), float(p), int(seed), int(offset), _p(y), _stream())
    return y


def dropout_mask(seed, offset, n, p, device="cuda"):
    """keep flags (uint8) of elements 0 .. n-1 of the Philox stream (seed, offset): what mm_dropout / mm_xattn_* apply (tests)."""
    m = torch.empty(n, dtype=torch.uint8, device=device)
    call("mm_dropout_mask", int(seed), int(offset), n, float(p), _p(m), _stream())
    return m


# ------------------------------------------------------------------------------------------------ activations
def swiglu_fwd(gu, I):
    M = gu.shape[0]
    out = torch.empty((M, I), dtype=gu.dtype, device=gu.device)
    call("mm_swiglu_fwd", dt(gu), _p(gu), M, I, _p(out), _stream())
    return out


def swiglu_bwd(gu, dout, I):
    dgu = torch.empty_like(gu)
    call("mm_swiglu_bwd", dt(gu), _p(gu), _p(dout), gu.shape[0], I, _p(dgu), _stream())
    return dgu


def xielu_fwd(x, alpha_p, alpha_n, beta, eps):
    """Apertus xIELU of the pre-activation x (any shape, contiguous).  alpha_p / alpha_n: the RAW one-element parameters (device
    memory, x's dtype); beta / eps: the values of the module's buffers as Python floats."""
    assert x.is_contiguous() and alpha_p.dtype == x.dtype and alpha_n.dtype == x.dtype
    y = torch.empty_like(x)
    call("mm_xielu_fwd", dt(x), _p(x), x.numel(), _p(alpha_p), _p(alpha_n), float(beta), float(eps), _p(y), _stream())
    return y


def xielu_bwd_blocks(n):
    return _lib.lib().mm_xielu_bwd_blocks(n)


def xielu_bwd(x, dy, alpha_p, alpha_n, beta, eps, want_dalpha=True):
    """-> (dx, partials): partials f32 [mm_xielu_bwd_blocks(n), 2] (the workgroups' sums for `xielu_reduce`), None when frozen."""
    assert x.is_contiguous() and dy.is_contiguous() and dy.dtype == x.dtype and dy.numel() == x.numel()
    dx = torch.empty_like(x)
    partials = torch.empty((xielu_bwd_blocks(x.numel()), 2), dtype=torch.float32, device=x.device) if want_dalpha else None
    call("mm_xielu_bwd", dt(x), _p(x), _p(dy), x.numel(), _p(alpha_p), _p(alpha_n), float(beta), float(eps), _p(dx), _p(partials), _stream())
    return dx, partials


def xielu_reduce(partials, alpha_p, alpha_n, dalpha_p, dalpha_n, accumulate_p, accumulate_n):
    """dalpha_*_raw (+)= softplus'(alpha_*_raw) * sum of the partials, fixed order, one rounding."""
    assert partials.is_contiguous() and dalpha_p.dtype == alpha_p.dtype and dalpha_n.dtype == alpha_n.dtype
    call("mm_xielu_reduce", dt(alpha_p), _p(partials), partials.shape[0], _p(alpha_p), _p(alpha_n), _p(dalpha_p), _p(dalpha_n),
         int(accumulate_p), int(accumulate_n), _stream())


def gelu_fwd(x, kind):
    y = torch.empty_like(x)
    call("mm_gelu_fwd", dt(x), kind, _p(x), x.numel(), _p(y), _stream())
    return y


def gelu_bwd(x, dy, kind):
    dx = torch.empty_like(x)
    call("mm_gelu_bwd", dt(x), kind, _p(x), _p(dy), x.numel(), _p(dx), _stream())
    return dx


def add(a, b):
    y = torch.empty_like(a)
    call("mm_add", dt(a), _p(a), _p(b), a.numel(), _p(y), _stream())
    return y


# ------------------------------------------------------------------------------------------------ loss
def ce_fwd(logits2d, V, labels):
    """logits2d: [T, ld] view with V valid columns.  -> (loss_and_count [2] f32, lse [T])."""
    T = logits2d.shape[0]
    ld = logits2d.stride(0)
    lse = torch.empty(T, dtype=torch.float32, device=logits2d.device)
    loss_row = torch.empty(T, dtype=torch.float32, device=logits2d.device)
    out = torch.empty(2, dtype=torch.float32, device=logits2d.device)
    call("mm_ce_fwd", dt(logits2d), _p(logits2d), T, V, ld, _p(labels), _p(lse), _p(loss_row), _stream())
    call("mm_ce_reduce", _p(loss_row), _p(labels), T, _p(out), _stream())
    return out, lse


def ce_bwd(logits2d, V, labels, lse, loss_and_count, gscale, dlogits2d):
    T = logits2d.shape[0]
    ld = logits2d.stride(0)
    assert dlogits2d.stride(0) == ld
    call("mm_ce_bwd", dt(logits2d), _p(logits2d), T, V, ld, _p(labels), _p(lse), _p(loss_and_count), _p(gscale), _p(dlogits2d),
         _stream())
    return dlogits2d


def argmax_softmax(logits2d, V, temperature):
    rows = logits2d.shape[0]
    out = torch.empty(rows, dtype=torch.int64, device=logits2d.device)
    if V >= 16384 and _on("MM_ARGMAX_SPLIT"):      # long rows: the vocabulary over many workgroups
        nb = _lib.lib().mm_argmax_softmax_ws_bytes(rows, V)
        ws = torch.empty((nb + 7) // 8, dtype=torch.int64, device=logits2d.device)
        call("mm_argmax_softmax_split", dt(logits2d), _p(logits2d), rows, V, logits2d.stride(0), float(temperature), _p(out), _p(ws), _stream())
        return out
    call("mm_argmax_softmax", dt(logits2d), _p(logits2d), rows, V, logits2d.stride(0), float(temperature), _p(out), _stream())
    return out


def _i64(v):
    """the 64-bit pattern of a Python int as a C int64_t (a seed may be given as any non-negative int below 2**64)"""
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >= 1 << 63 else v


def sample_ws(rows, V, device):
    """workspace of mm_sample for `rows` rows of V logits (reusable across calls of that size)."""
    return torch.empty((_sizes("mm_sample_ws_bytes", int(rows), int(V)) + 15) // 16 * 2, dtype=torch.int64, device=device)


def sample(logits2d, V, temperature, top_k=0, top_p=1.0, min_p=0.0, seed=0, offset=0, thresh=False, ws=None, out=None):
    """seeded temperature -> top-k -> top-p -> min-p draw per row (contract: mm_sample in include/mm_hip.h).  Returns the
    int64 token ids [rows], or (ids, smallest kept x per row) when thresh.  ws: sample_ws(rows, V, device), owned by the caller."""
    rows = logits2d.shape[0]
    assert logits2d.stride(-1) == 1
    if ws is None:
        ws = sample_ws(rows, V, logits2d.device)
    if out is None:
        out = torch.empty(rows, dtype=torch.int64, device=logits2d.device)
    th = torch.empty(rows, dtype=torch.float32, device=logits2d.device) if thresh else None
    call("mm_sample", dt(logits2d), _p(logits2d), rows, V, logits2d.stride(0), float(temperature), min(int(top_k), V), float(top_p),
         float(min_p), _i64(seed), _i64(offset), _p(out), _p(th), _p(ws), ws.numel() * 8, _stream())
    return (out, th) if thresh else out


def sample_uniforms(seed, offset, rows, device="cuda"):
    """the uniforms u of mm_sample's draws for rows 0 .. rows-1 (tests)."""
    u = torch.empty(rows, dtype=torch.float32, device=device)
    call("mm_sample_uniforms", _i64(seed), _i64(offset), rows, _p(u), _stream())
    return u


def expert_fuse(x, gate, idx, mode, backward=False, E=None):
    """MoE fusion (see mm_expert_fuse).  forward: x [E, n, L] -> [n, L] (mode 0) / [n, J, L] (mode 1); backward: x = dout ->
    dX [E, n, L] (zeros outside the listed experts)."""
    J = len(idx)
    ix = (ctypes.c_int * J)(*[int(i) for i in idx])
    if not backward:
        E_, n, L = x.shape
        out = torch.empty((n, L) if mode == 0 else (n, J, L), dtype=x.dtype, device=x.device)
    else:
        E_ = int(E)
        n, L = x.shape[0], x.shape[-1]
        out = torch.zeros((E_, n, L), dtype=x.dtype, device=x.device)
    call("mm_expert_fuse", dt(x), int(backward), int(mode), _p(x), _p(gate), ix, J, E_, n, L, _p(out), _stream())
    return out


def decode_select(tok, finished, eos, out, col, next_ids):
    """device-side eos bookkeeping of one decode step (no host sync): see mm_decode_select."""
    call("mm_decode_select", _p(tok), _p(finished), int(eos), tok.numel(), _p(out), out.stride(0), int(col), _p(next_ids), _stream())


def prompt_history(prompt_ids, prompt_mask, samples=1, room=0):
    """The rows' id history as mm_logits_process and mm_lookup_draft read it: (hist int32 [B samples, Sp + room] -- a row's prompt ids
    where the mask is not 0, in order, then -1 --, plen int32 [B samples], Sp).  Every prompt row is repeated `samples` times."""
    B, Sp = prompt_ids.shape
    device = prompt_ids.device
    assert prompt_mask.shape == prompt_ids.shape
    keep = prompt_mask != 0
    order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)              # the visible positions first, in order
    plen = keep.sum(dim=1)
    ids = torch.gather(prompt_ids, 1, order).masked_fill(torch.arange(Sp, device=device)[None, :] >= plen[:, None], -1)
    hist = torch.full((B, Sp + int(room)), -1, dtype=torch.int32, device=device)
    hist[:, :Sp] = ids.to(torch.int32)
    if samples > 1:
        hist = hist.repeat_interleave(samples, dim=0).contiguous()
    return hist, plen.to(torch.int32).repeat_interleave(samples).contiguous(), int(Sp)


class LogitsState:
    """The device state of generate()'s logits processors for one call: the settings, the suppressed ids (int32), the fp32 score
    rows the selectors read, and -- only when the repetition penalty or the n-gram ban is on -- the int32 history of every row
    (mm_logits_process: the row's prompt ids first, then the emitted ids, appended by the kernel).

    prompt_ids / prompt_mask [B, Sp] (device): a row's prompt history is its ids where the mask is not 0, in order; every prompt row
    is repeated `samples` times (row b samples + j).  room = the number of steps the history must hold."""

    def __init__(self, rows, V, device, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress=(), prompt_ids=None,
                 prompt_mask=None, samples=1, room=0):
        self.rows, self.V = int(rows), int(V)
        self.p, self.g, self.min_new = float(repetition_penalty), int(no_repeat_ngram_size), int(min_new_tokens)
        self.suppress = torch.tensor([int(t) for t in suppress], dtype=torch.int32, device=device) if len(suppress) else None
        self.ld_out = (self.V + 63) // 64 * 64
        self.out = torch.empty((self.rows, self.ld_out), dtype=torch.float32, device=device)
        self.hist = self.plen = None
        self.max_plen = 0
        if self.p != 1.0 or self.g > 0:
            assert prompt_ids.shape[0] * samples == self.rows
            self.hist, self.plen, self.max_plen = prompt_history(prompt_ids, prompt_mask, samples, room)


def logits_process(logits2d, st: LogitsState, step, last_ids, eos):
    """rules 1-5 of mm_logits_process on logits [rows, >= V] (bf16 / fp32) -> st.out[:, :V] (fp32, what the selectors read);
    last_ids: the ids the previous step emitted (read when step > 0 and a history is kept)."""
    assert logits2d.stride(-1) == 1 and logits2d.shape[0] == st.rows
    hist = st.hist
    call("mm_logits_process", dt(logits2d), _p(logits2d), st.rows, st.V, logits2d.stride(0), int(step),
         _p(last_ids) if hist is not None else None, _p(hist), hist.stride(0) if hist is not None else 0, _p(st.plen), st.max_plen,
         st.p, st.g, st.min_new, int(eos), _p(st.suppress), 0 if st.suppress is None else st.suppress.numel(), _p(st.out), st.ld_out,
         _stream())
    return st.out[:, :st.V]


class GuidanceState:
    """The device state of generate(guidance_scale=) for one call: mm_cfg_combine's workspace (the chunk partials of 2 rows log-sum-exp)
    and the fp32 score rows [rows, V] (row stride padded to 64) the processors and selectors read.  rows = the number of
    (conditional, unconditional) pairs."""

    def __init__(self, rows, V, device):
        self.rows, self.V = int(rows), int(V)
        self.ws_bytes = _sizes("mm_cfg_ws_bytes", self.rows, self.V)
        self.ws = torch.empty(max(1, (self.ws_bytes + 15) // 16) * 2, dtype=torch.int64, device=device)
        self.ld_out = (self.V + 63) // 64 * 64
        self.out = torch.empty((self.rows, self.ld_out), dtype=torch.float32, device=device)


def cfg_combine(logits2d, st: GuidanceState, scale):
    """mm_cfg_combine on ONE logits tensor [2 rows, >= V] (bf16 / fp32) of a guided decoder pass: rows [0, rows) are the conditional
    ones, rows [rows, 2 rows) their unconditional partners -> st.out[:, :V], fp32 scores = log_softmax(uncond) + scale *
    (log_softmax(cond) - log_softmax(uncond))."""
    assert logits2d.stride(-1) == 1 and logits2d.shape[0] == 2 * st.rows and logits2d.shape[1] >= st.V
    ld = logits2d.stride(0)
    call("mm_cfg_combine", dt(logits2d), _p(logits2d), ld, _p(logits2d[st.rows:]) if st.rows else _p(logits2d), ld, st.rows, st.V,
         float(scale), _p(st.out), st.ld_out, _p(st.ws), st.ws_bytes, _stream())
    return st.out[:, :st.V]


# ---- prompt-lookup speculative decoding (include/mm_hip.h: mm_lookup_draft, mm_kv_append_at, mm_lookup_accept) ----
class LookupState:
    """The device state of generate(prompt_lookup_num_tokens=k) for one call: per row the int32 history (prompt_history's layout: the
    visible prompt ids, then every emitted id) with its length hlen, the emitted count, the finished flag, `base` (position and cache
    slot of the row's newest id; LayerKVCacheLookup reads the same tensor), the stats (verify steps, accepted drafts) and one done
    flag; the step's ids / position_ids / n_draft and the output ids [rows, max_new] (eos-filled)."""

    def __init__(self, prompt_ids, prompt_mask, k, max_ngram, max_new, eos, base0):
        dev = prompt_ids.device
        self.rows, self.k, self.Q, self.G, self.max_new, self.eos = int(prompt_ids.shape[0]), int(k), int(k) + 1, int(max_ngram), int(max_new), int(eos)
        self.hist, self.hlen, _ = prompt_history(prompt_ids, prompt_mask, 1, self.max_new)
        z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        self.count, self.finished, self.n_draft, self.stats, self.done = z(self.rows), z(self.rows), z(self.rows), z(self.rows, 2), z(1)
        self.base = torch.full((self.rows,), int(base0), dtype=torch.int32, device=dev)
        self.ids = torch.zeros((self.rows, self.Q), dtype=torch.int64, device=dev)
        self.pos = torch.zeros((self.rows, self.Q), dtype=torch.int64, device=dev)
        self.out = torch.full((self.rows, self.max_new), self.eos, dtype=torch.int64, device=dev)


def lookup_draft(st: LookupState):
    """mm_lookup_draft: st.ids / st.pos [rows, k+1] and st.n_draft of the coming verify step, from the rows' histories."""
    call("mm_lookup_draft", _p(st.hist), st.hist.stride(0), _p(st.hlen), _p(st.count), _p(st.finished), _p(st.base), st.rows, st.k, st.G,
         st.max_new, st.eos, _p(st.ids), _p(st.pos), _p(st.n_draft), _stream())
    return st.ids, st.pos


def lookup_accept(st: LookupState, tok, Q=None):
    """mm_lookup_accept of the selector's tok [rows * Q] (Q = k + 1; Q = 1: the prefill's token, no drafts): emits, appends to the
    history and advances count / hlen / base / stats / done."""
    Q = st.Q if Q is None else int(Q)
    assert tok.dtype == torch.int64 and tok.numel() == st.rows * Q and tok.is_contiguous()
    call("mm_lookup_accept", _p(tok), _p(st.ids) if Q > 1 else None, _p(st.n_draft) if Q > 1 else None, st.rows, Q, st.max_new, st.eos,
         _p(st.out), st.out.stride(0), _p(st.hist), st.hist.stride(0), _p(st.hlen), _p(st.count), _p(st.finished), _p(st.base),
         _p(st.stats), _p(st.done), _stream())


def lookup_append(qkv, B, Q, Hq, Hkv, D, base, kcache, vcache):
    """mm_kv_append_at: the (roped) k and the v heads of qkv [B*Q, (Hq+2Hkv)*D] -> cache[b, base[b] + j] (a pure copy; a slot past the
    cache is skipped)."""
    assert qkv.shape[0] == B * Q and qkv.stride(1) == 1 and base.dtype == torch.int32 and base.numel() == B
    assert kcache.stride(3) == 1 and kcache.stride(2) == D and vcache.stride() == kcache.stride() and kcache.shape[0] == B
    call("mm_kv_append_at", dt(qkv), _p(qkv), qkv.stride(0), B, Q, Hq, Hkv, D, _p(base), _p(kcache), _p(vcache), kcache.stride(0),
         kcache.stride(1), kcache.shape[1], _stream())


def attn_decode_verify(q, k, v, Q, key_mask, base, scale, nsplit=None):
    """Q causal query positions per sequence: q [B*Q,Hq,D] (strided view ok; row b*Q + j) over k/v [B,Scap,Hkv,D], query (b, j) seeing
    keys t <= base[b] + j (base int32 [B] on the device) minus the prompt keys key_mask [B,Sp] hides -> out [B*Q,Hq,D].  The bits of
    attn_decode per row under the equivalent mask (mm_attn_decode_verify)."""
    R, Hq, D = q.shape
    B, Scap, Hkv = k.shape[0], k.shape[1], k.shape[2]
    assert R == B * Q and v.shape[:3] == k.shape[:3] and q.stride(2) == 1 and k.stride(3) == 1 and v.stride(3) == 1
    assert base.dtype == torch.int32 and base.numel() == B and base.is_contiguous()
    assert key_mask is None or (key_mask.dim() == 2 and key_mask.shape[0] == B and key_mask.is_contiguous() and key_mask.dtype == torch.int64)
    ns = _lib.lib().mm_attn_decode_verify_splits(B, Q, Hkv, Scap) if nsplit is None else int(nsplit)
    ws, out = _decode_ws(q, ns)
    call("mm_attn_decode_verify", dt(q), _p(q), _p(k), _p(v), B, Q, Scap, 0 if key_mask is None else key_mask.shape[1], Hq, Hkv, D,
         q.stride(0), q.stride(1), *_strides3(k), *_strides3(v), _p(key_mask), _p(base), float(scale), _p(out), _p(ws), ns, _stream())
    return out


# ------------------------------------------------------------------------------------------------ optimizer
def gradnorm(flat_grads, max_norm):
    """flat_grads: list of 1-D flat gradient buffers -> device tensor [2] = (total_norm, clip_coef)."""
    nblk = 1024
    dev = flat_grads[0].device
    partial = torch.empty(nblk * len(flat_grads), dtype=torch.float32, device=dev)
    for i, g in enumerate(flat_grads):
        call("mm_gradnorm_partial", dt(g), _p(g), g.numel(), partial.data_ptr() + 4 * nblk * i, nblk, _stream())
    total = torch.empty(2, dtype=torch.float32, device=dev)
    call("mm_gradnorm_finish", _p(partial), nblk * len(flat_grads), float(max_norm), _p(total), _stream())
    return total


def gradnorm_partial(g, partial):
    """sum of squares of one flat gradient slice -> partial[:] (one float per workgroup; any stream)."""
    call("mm_gradnorm_partial", dt(g), _p(g), g.numel(), _p(partial), partial.numel(), _stream())


def gradnorm_finish(partial, max_norm):
    """-> device tensor [2] = (total_norm, clip_coef) from all the partial slots, summed in slot order (deterministic)."""
    total = torch.empty(2, dtype=torch.float32, device=partial.device)
    call("mm_gradnorm_finish", _p(partial), partial.numel(), float(max_norm), _p(total), _stream())
    return total


def adamw_step(p, g, master, m, v, lr, beta1, beta2, eps, wd, step, clip=None):
    call("mm_adamw_step", dt(p), _p(p), _p(g), _p(master), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2),
         float(eps), float(wd), int(step), _p(clip), _stream())


def adamw_step_split(p, g, lo, m, v, lr, beta1, beta2, eps, wd, step, clip=None):
    """AdamW on (bf16 parameter, int16 remainder) = the fp32 master in two halves (mm_adamw_step_split): 26 B per parameter."""
    assert p.dtype == torch.bfloat16 and g.dtype == torch.bfloat16 and lo.dtype == torch.int16
    call("mm_adamw_step_split", _p(p), _p(g), _p(lo), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps), float(wd),
         int(step), _p(clip), _stream())


def master_split(master, p, lo):
    """fp32 master -> p = RNE(master) (bf16) and the int16 remainder lo."""
    call("mm_master_split", _p(master), master.numel(), _p(p), _p(lo), _stream())


def master_join(p, lo):
    """(bf16 parameter, int16 remainder) -> the fp32 master they encode."""
    out = torch.empty(p.numel(), dtype=torch.float32, device=p.device)
    call("mm_master_join", _p(p), _p(lo), p.numel(), _p(out), _stream())
    return out


def cast(src, dtype):
    dst = torch.empty(src.shape, dtype=dtype, device=src.device)
    call("mm_cast", dt(src), _DT[dtype], _p(src), _p(dst), src.numel(), _stream())
    return dst



# ------------------------------------------------------------------------------------------------ gating network (NHWC conv)
def nchw_to_nhwc(pixels: torch.Tensor, cpad: int, dtype: torch.dtype) -> torch.Tensor:
    """fp32 pixels [n, C, H, W] -> [n, H, W, cpad] in `dtype`, channels C .. cpad-1 zero."""
    assert pixels.dtype == torch.float32 and pixels.dim() == 4 and pixels.is_contiguous()
    n, C, H, W = pixels.shape
    out = torch.empty((n, H, W, cpad), dtype=dtype, device=pixels.device)
    call("mm_nchw_to_nhwc", _DT[dtype], _p(pixels), n, C, H, W, cpad, _p(out), _stream())
    return out


def conv_out_size(size: int, R: int, stride: int, pad: int) -> int:
    return (size + 2 * pad - R) // stride + 1


def conv2d_nhwc(x: torch.Tensor, w: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, stride: int, pad: int,
                residual: Optional[torch.Tensor] = None, relu: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y [n, Ho, Wo, Cout] = act(conv(x [n, H, W, Cin], w [Cout, R, R, Cin]) * scale + shift (+ residual)); scale / shift fp32."""
    assert x.dim() == 4 and w.dim() == 4 and x.is_contiguous() and w.is_contiguous() and w.dtype == x.dtype
    n, H, W, Cin = x.shape
    Cout, R = w.shape[0], w.shape[1]
    assert w.shape[2] == R and w.shape[3] == Cin and scale.dtype == torch.float32 and shift.dtype == torch.float32
    Ho, Wo = conv_out_size(H, R, stride, pad), conv_out_size(W, R, stride, pad)
    if out is None:
        out = torch.empty((n, Ho, Wo, Cout), dtype=x.dtype, device=x.device)
    if residual is not None:
        assert residual.shape == out.shape and residual.is_contiguous() and residual.dtype == x.dtype
    call("mm_conv2d_nhwc_fwd", dt(x), _p(x), n, H, W, Cin, _p(w), Cout, R, stride, pad, _p(scale), _p(shift), _p(residual),
         int(relu), _p(out), _stream())
    return out


def maxpool2d_nhwc(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """3x3 / stride 2 / pad 1 max pool on [n, H, W, C]."""
    assert x.dim() == 4 and x.is_contiguous()
    n, H, W, C = x.shape
    if out is None:
        out = torch.empty((n, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), dtype=x.dtype, device=x.device)
    call("mm_maxpool2d_nhwc", dt(x), _p(x), n, H, W, C, _p(out), _stream())
    return out


def gate_head(x: torch.Tensor, fc_w: torch.Tensor, fc_b: torch.Tensor, top_k: int):
    """x [n, HW, C] -> (logits [n, E], topk_idx int64 [n, top_k], weights [n, E]): mean over HW, fc, softmax, top-k in one launch."""
    assert x.dim() == 3 and x.is_contiguous() and fc_w.is_contiguous() and fc_w.dtype == x.dtype and fc_b.dtype == x.dtype
    n, HW, C = x.shape
    E = fc_w.shape[0]
    logits = torch.empty((n, E), dtype=x.dtype, device=x.device)
    weights = torch.empty((n, E), dtype=x.dtype, device=x.device)
    topk = torch.empty((n, top_k), dtype=torch.int64, device=x.device)
    call("mm_gate_head", dt(x), _p(x), n, HW, C, _p(fc_w), _p(fc_b), E, top_k, _p(logits), _p(weights), _p(topk), _stream())
    return logits, topk, weights


# ------------------------------------------------------------------------------------------------ gating network, training pieces
def bn_train_ws(M: int, C: int, device) -> torch.Tensor:
    """the fp32 workspace of bn_train_fwd / bn_train_bwd for z [M, C]."""
    return torch.empty(_sizes("mm_bn_train_ws_bytes", int(M), int(C)) // 4, dtype=torch.float32, device=device)


def bn_train_fwd(z: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, residual: Optional[torch.Tensor] = None, relu: bool = False,
                 eps: float = 1e-5, momentum: float = 0.1, running_mean: Optional[torch.Tensor] = None,
                 running_var: Optional[torch.Tensor] = None, num_batches_tracked: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None, mean: Optional[torch.Tensor] = None, invstd: Optional[torch.Tensor] = None,
                 ws: Optional[torch.Tensor] = None):
    """BatchNorm with batch statistics on z [..., C] (rows = every leading dimension): -> (y, mean fp32 [C], invstd fp32 [C]);
    the running statistics, when given, are updated in place (see mm_bn_train_fwd)."""
    assert z.is_contiguous() and gamma.dtype == z.dtype and beta.dtype == z.dtype and gamma.is_contiguous() and beta.is_contiguous()
    C = z.shape[-1]
    M = z.numel() // C
    if out is None:
        out = torch.empty_like(z)
    if mean is None:
        mean = torch.empty(C, dtype=torch.float32, device=z.device)
    if invstd is None:
        invstd = torch.empty(C, dtype=torch.float32, device=z.device)
    if ws is None:
        ws = bn_train_ws(M, C, z.device)
    if residual is not None:
        assert residual.shape == z.shape and residual.is_contiguous() and residual.dtype == z.dtype
    if running_mean is not None:
        assert running_mean.dtype == z.dtype and running_var.dtype == z.dtype and num_batches_tracked.dtype == torch.int64
    call("mm_bn_train_fwd", dt(z), _p(z), M, C, _p(gamma), _p(beta), _p(residual), int(relu), float(eps), float(momentum), _p(out),
         _p(mean), _p(invstd), _p(running_mean), _p(running_var), _p(num_batches_tracked), _p(ws), ws.numel() * 4, _stream())
    return out, mean, invstd


def bn_train_bwd(dy: torch.Tensor, y: Optional[torch.Tensor], z: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor,
                 gamma: torch.Tensor, relu: bool, want_dres: bool = False, dz: Optional[torch.Tensor] = None,
                 dres: Optional[torch.Tensor] = None, dgamma: Optional[torch.Tensor] = None, dbeta: Optional[torch.Tensor] = None,
                 ws: Optional[torch.Tensor] = None):
    """-> (dz, dres or None, dgamma, dbeta) of bn_train_fwd (see mm_bn_train_bwd); y is the forward's output (the ReLU mask)."""
    assert dy.is_contiguous() and z.is_contiguous() and dy.shape == z.shape and dy.dtype == z.dtype and gamma.dtype == z.dtype
    assert mean.dtype == torch.float32 and invstd.dtype == torch.float32 and (not relu or (y is not None and y.is_contiguous()))
    C = z.shape[-1]
    M = z.numel() // C
    if dz is None:
        dz = torch.empty_like(z)
    if dres is None and want_dres:
        dres = torch.empty_like(z)
    if dgamma is None:
        dgamma = torch.empty(C, dtype=z.dtype, device=z.device)
    if dbeta is None:
        dbeta = torch.empty(C, dtype=z.dtype, device=z.device)
    if ws is None:
        ws = bn_train_ws(M, C, z.device)
    call("mm_bn_train_bwd", dt(z), _p(dy), _p(y), _p(z), M, C, _p(mean), _p(invstd), _p(gamma), int(relu), _p(dz), _p(dres), _p(dgamma),
         _p(dbeta), _p(ws), ws.numel() * 4, _stream())
    return dz, dres, dgamma, dbeta


def maxpool2d_nhwc_bwd(x: torch.Tensor, dy: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dx of the 3x3 / stride 2 / pad 1 max pool: x [n, H, W, C] is the forward's input, dy [n, Ho, Wo, C]."""
    assert x.dim() == 4 and x.is_contiguous() and dy.is_contiguous() and dy.dtype == x.dtype
    n, H, W, C = x.shape
    assert dy.shape == (n, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C)
    if out is None:
        out = torch.empty_like(x)
    call("mm_maxpool2d_nhwc_bwd", dt(x), _p(x), _p(dy), n, H, W, C, _p(out), _stream())
    return out


def expert_fuse_gate_bwd(x, dout, gate, idx, mode, out=None):
    """d(loss) / d(gate) of expert_fuse: x [E, n, L], dout [n, L] (mode 0) / [n, J, L] (mode 1), gate [n, E] fp32 -> fp32 [n, E]."""
    J = len(idx)
    E_, n, L = x.shape
    assert x.is_contiguous() and dout.is_contiguous() and dout.dtype == x.dtype and gate.dtype == torch.float32 and gate.is_contiguous()
    assert dout.shape == ((n, L) if mode == 0 else (n, J, L)) and gate.shape == (n, E_)
    ix = (ctypes.c_int * J)(*[int(i) for i in idx])
    b = _sizes("mm_expert_fuse_gate_bwd_ws_bytes", dt(x), J, n, L)
    ws = torch.empty(b // 4, dtype=torch.float32, device=x.device)
    if out is None:
        out = torch.empty((n, E_), dtype=torch.float32, device=x.device)
    call("mm_expert_fuse_gate_bwd", dt(x), int(mode), _p(x), _p(dout), _p(gate), ix, J, E_, n, L, _p(out), _p(ws), b, _stream())
    return out


def conv2d_nhwc_dgrad(dz: torch.Tensor, wp: torch.Tensor, H: int, W: int, stride: int, pad: int, addend: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dx [n, H, W, Cin] of conv2d_nhwc from dz [n, Ho, Wo, Cout] and the filter packed [Cin, R, R, Cout] (+ addend, in fp32)."""
    assert dz.dim() == 4 and wp.dim() == 4 and dz.is_contiguous() and wp.is_contiguous() and wp.dtype == dz.dtype
    n, Ho, Wo, Cout = dz.shape
    Cin, R = wp.shape[0], wp.shape[1]
    assert wp.shape[2] == R and wp.shape[3] == Cout
    assert (Ho, Wo) == (conv_out_size(H, R, stride, pad), conv_out_size(W, R, stride, pad))
    if out is None:
        out = torch.empty((n, H, W, Cin), dtype=dz.dtype, device=dz.device)
    if addend is not None:
        assert addend.shape == out.shape and addend.is_contiguous() and addend.dtype == dz.dtype
    call("mm_conv2d_nhwc_dgrad", dt(dz), _p(dz), n, H, W, Cin, _p(wp), Cout, R, stride, pad, _p(addend), _p(out), _stream())
    return out


def conv2d_nhwc_wgrad_ws_bytes(n: int, H: int, W: int, Cin: int, Cout: int, R: int, stride: int, pad: int) -> int:
    return _sizes("mm_conv2d_nhwc_wgrad_ws_bytes", n, H, W, Cin, Cout, R, stride, pad)


def conv2d_nhwc_wgrad(dz: torch.Tensor, x: torch.Tensor, R: int, stride: int, pad: int, out: Optional[torch.Tensor] = None,
                      ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dw [Cout, R, R, Cin] (the forward's packed order) of conv2d_nhwc from dz [n, Ho, Wo, Cout] and the input x [n, H, W, Cin]."""
    assert dz.dim() == 4 and x.dim() == 4 and dz.is_contiguous() and x.is_contiguous() and x.dtype == dz.dtype
    n, H, W, Cin = x.shape
    Cout = dz.shape[3]
    assert dz.shape == (n, conv_out_size(H, R, stride, pad), conv_out_size(W, R, stride, pad), Cout)
    if out is None:
        out = torch.empty((Cout, R, R, Cin), dtype=x.dtype, device=x.device)
    if ws is None:
        ws = torch.empty(conv2d_nhwc_wgrad_ws_bytes(n, H, W, Cin, Cout, R, stride, pad) // 4, dtype=torch.float32, device=x.device)
    call("mm_conv2d_nhwc_wgrad", dt(x), _p(dz), _p(x), n, H, W, Cin, Cout, R, stride, pad, _p(out), _p(ws), ws.numel() * 4, _stream())
    return out
