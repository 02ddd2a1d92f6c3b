#!/usr/bin/env python3
"""Small HBM-bound kernels in isolation at the shapes of the 8B step (decoder rows 8192 x 4096, ViT-L rows 1028 x 1024/4096):
time per launch and the bytes each must move, so that an in-step duration (rocprofv3, other streams sharing the chip) can be
told from the kernel's own speed.  Also Qwen3's fused per-head q/k RMSNorm + RoPE at the Qwen3-4B step's shape, and the two MLP
activations at Apertus-8B width (M = 8192, I = 21504): SwiGLU and xIELU, forward and backward."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from multimeditron_amd import kernels as K


def timeit(name, fn, nbytes, it=50):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(it):
        fn()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / it * 1e3
    print(f"{name:44s} {us:8.1f} us   {nbytes / 1e6:8.1f} MB   {nbytes / us / 1e6:7.2f} TB/s", flush=True)


def main():
    dev = "cuda"
    bf = torch.bfloat16
    for M, H, tag in ((8192, 4096, "decoder"), (1028, 1024, "vit")):
        x = torch.randn(M, H, device=dev).to(bf)
        dy = torch.randn(M, H, device=dev).to(bf)
        w = torch.randn(H, device=dev).to(bf)
        b = torch.randn(H, device=dev).to(bf)
        if tag == "decoder":
            y, rstd = K.rmsnorm_fwd(x, w, 1e-5)
            timeit(f"rmsnorm_fwd {M}x{H}", lambda: K.rmsnorm_fwd(x, w, 1e-5), 2 * M * H * 2)
            timeit(f"rmsnorm_bwd {M}x{H} (+dres)", lambda: K.rmsnorm_bwd(dy, x, w, rstd, dy), 4 * M * H * 2)
            dx, dwp = K.rmsnorm_bwd(dy, x, w, rstd, dy)
        else:
            y, mean, rstd = K.layernorm_fwd(x, w, b, 1e-5)
            timeit(f"layernorm_fwd {M}x{H}", lambda: K.layernorm_fwd(x, w, b, 1e-5), 2 * M * H * 2)
            timeit(f"layernorm_bwd {M}x{H} (+dres)", lambda: K.layernorm_bwd(dy, x, w, mean, rstd, dy), 4 * M * H * 2)
            dx, dwp, dbp = K.layernorm_bwd(dy, x, w, mean, rstd, dy)
        out = torch.zeros(H, device=dev, dtype=bf)
        timeit(f"reduce_partials {dwp.shape[0]}x{H}", lambda: K.reduce_partials(dwp, out, True), dwp.numel() * 4)
    for M, N in ((1028, 1024), (1028, 4096), (1028, 3072)):
        x = torch.randn(M, N, device=dev).to(bf)
        out = torch.zeros(N, device=dev, dtype=bf)
        timeit(f"colsum {M}x{N}", lambda: K.colsum(x, out, False), M * N * 2)
    x = torch.randn(1028, 4096, device=dev).to(bf)
    timeit("gelu_fwd(quick) 1028x4096", lambda: K.gelu_fwd(x, 1), 2 * x.numel() * 2)
    timeit("gelu_bwd(quick) 1028x4096", lambda: K.gelu_bwd(x, x, 1), 3 * x.numel() * 2)
    # Qwen3's per-head q/k norm + RoPE at the 4B step's shape (T = 8192 tokens, 32 + 8 heads x 128 inside a 48-head qkv row),
    # next to the RoPE alone on the same heads (the Llama path's separate pass)
    T, Hq, Hkv, D = 8192, 32, 8, 128
    nh, W = Hq + Hkv, (Hq + 2 * Hkv) * D
    qkv = torch.randn(T, W, device=dev).to(bf)
    wq, wk = torch.ones(D, device=dev, dtype=bf), torch.ones(D, device=dev, dtype=bf)
    cos, sin = K.rope_table(torch.arange(T, device=dev), torch.rand(D // 2, device=dev), True)
    qk, rstd = K.qk_norm_rope_fwd(qkv, T, Hq, Hkv, D, wq, wk, 1e-6, cos, sin)
    tab = 2 * T * (D // 2) * 4
    timeit(f"qk_norm_rope_fwd {T}x{nh}x{D}", lambda: K.qk_norm_rope_fwd(qkv, T, Hq, Hkv, D, wq, wk, 1e-6, cos, sin, out=qk),
           2 * T * nh * D * 2 + T * nh * 4 + tab)
    dqkv = torch.empty_like(qkv)
    timeit(f"qk_norm_rope_bwd {T}x{nh}x{D}", lambda: K.qk_norm_rope_bwd(qk, qkv, T, Hq, Hkv, D, wq, wk, rstd, cos, sin, dqkv),
           3 * T * nh * D * 2 + T * nh * 4 + tab)
    dwq, _ = K.qk_norm_rope_bwd(qk, qkv, T, Hq, Hkv, D, wq, wk, rstd, cos, sin, dqkv)
    out = torch.zeros(D, device=dev, dtype=bf)
    timeit(f"reduce_partials {dwq.shape[0]}x{D} (x2 per layer)", lambda: K.reduce_partials(dwq, out, True), dwq.numel() * 4)
    timeit(f"rope_apply {T}x{nh}x{D} (Llama path)", lambda: K.rope_apply_(qkv, T, nh, D, W, cos, sin), 2 * T * nh * D * 2 + tab)
    # the MLP activations at Apertus-8B width: SwiGLU reads gate | up (2 I) and writes I; xIELU reads and writes I (its backward
    # also leaves the two scalar gradients' partial sums, finished by xielu_reduce)
    M, I = 8192, 21504
    gu = torch.randn(M, 2 * I, device=dev).to(bf)
    d = torch.randn(M, I, device=dev).to(bf)
    timeit(f"swiglu_fwd {M}x{I}", lambda: K.swiglu_fwd(gu, I), 3 * M * I * 2, it=20)
    timeit(f"swiglu_bwd {M}x{I}", lambda: K.swiglu_bwd(gu, d, I), 5 * M * I * 2, it=20)
    del gu
    u = torch.randn(M, I, device=dev).to(bf)
    ap_, an_ = torch.full((1,), 0.2041, device=dev, dtype=bf), torch.full((1,), -1.0469, device=dev, dtype=bf)
    beta, eps = 0.5, float(torch.tensor(-1e-6, dtype=bf))
    timeit(f"xielu_fwd {M}x{I}", lambda: K.xielu_fwd(u, ap_, an_, beta, eps), 2 * M * I * 2, it=20)
    timeit(f"xielu_bwd {M}x{I} (+ partial sums)", lambda: K.xielu_bwd(u, d, ap_, an_, beta, eps), 3 * M * I * 2, it=20)
    timeit(f"xielu_bwd {M}x{I} (frozen scalars)", lambda: K.xielu_bwd(u, d, ap_, an_, beta, eps, want_dalpha=False), 3 * M * I * 2, it=20)
    _, part = K.xielu_bwd(u, d, ap_, an_, beta, eps)
    gp, gn = torch.zeros(1, device=dev, dtype=bf), torch.zeros(1, device=dev, dtype=bf)
    timeit(f"xielu_reduce {part.shape[0]}x2", lambda: K.xielu_reduce(part, ap_, an_, gp, gn, False, False), part.numel() * 4)
    del u, d
    x = torch.empty(1 << 28, device=dev, dtype=bf)
    timeit("torch zero_ 512 MB", lambda: x.zero_(), x.numel() * 2, it=10)


if __name__ == "__main__":
    main()
