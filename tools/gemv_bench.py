#!/usr/bin/env python3
"""The decode step's weight-streaming kernels one by one at the 8B decoder's shapes (B rows of activations), each timed over L
different layers' weights (L x 436 MB: far beyond the 256 MB Infinity Cache, as in a real token) -- us per launch and TB/s of
weight bytes, first on the bf16 weights and then on their weight-only MXFP8 copies (the bytes actually read: 1 + 1/32 per weight
plus the layout's padding).  The attention launch and the S = 1 cache append are timed over the bf16 cache and over its MXFP8 form
(the bytes actually read: 132 per head row against 256).   python tools/gemv_bench.py [B] [L]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from multimeditron_amd import kernels as K

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
L = int(sys.argv[2]) if len(sys.argv) > 2 else 16
H, I, Hq, Hkv, D, S = 4096, 14336, 32, 8, 128, 2048
dev = "cuda"
torch.manual_seed(0)
bf = torch.bfloat16
w_qkv = [torch.randn((Hq + 2 * Hkv) * D, H, device=dev, dtype=bf) * 0.02 for _ in range(L)]
w_o = [torch.randn(H, H, device=dev, dtype=bf) * 0.02 for _ in range(L)]
w_gu = [torch.randn(2 * I, H, device=dev, dtype=bf) * 0.02 for _ in range(L)]
w_d = [torch.randn(H, I, device=dev, dtype=bf) * 0.02 for _ in range(L)]
kc = [torch.randn(B, S + 8, Hkv, D, device=dev, dtype=bf) for _ in range(L)]
vc = [torch.randn(B, S + 8, Hkv, D, device=dev, dtype=bf) for _ in range(L)]
nw = torch.ones(H, device=dev, dtype=bf)
x = torch.randn(B, H, device=dev, dtype=bf)
act = torch.randn(B, I, device=dev, dtype=bf)
q = torch.randn(B, Hq, D, device=dev, dtype=bf)
cos = torch.randn(B, 64, device=dev)
sin = torch.randn(B, 64, device=dev)


def timed(name, fn, bytes_per_call, reps=6):
    for i in range(L):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        for i in range(L):
            fn(i)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / (reps * L)
    print(f"{name:34s} {us:7.1f} us/launch   {bytes_per_call / us / 1e6:5.2f} TB/s   ({bytes_per_call / 1e6:.0f} MB)", flush=True)
    return us


nw2 = torch.ones(I, device=dev, dtype=bf)
from multimeditron_amd._lib import lib
for nt in (0, 1):
    lib().mm_set_option(b"gemv_nt", nt)
    print(f"-- weight loads: {'non-temporal' if nt else 'default policy'}")
    tot = 0.0
    tot += timed("norm + q|k|v + RoPE + append (N=6144)", lambda i: K.decode_qkv_rope_append(x, w_qkv[i], None, Hq, Hkv, D, cos, sin, kc[i], vc[i], S, norm_w=nw, eps=1e-5), w_qkv[0].numel() * 2)
    tot += timed("attention partial+merge (S=2048)", lambda i: K.attn_decode(q, kc[i][:, :S], vc[i][:, :S], None, D ** -0.5), 2 * B * S * Hkv * D * 2)
    tot += timed("o_proj + residual (N=4096)", lambda i: K.decode_linear(x, w_o[i], residual=x), w_o[0].numel() * 2)
    tot += timed("norm + gate|up + SwiGLU (N=2x14336)", lambda i: K.decode_gateup_swiglu(x, w_gu[i], I, norm_w=nw, eps=1e-5), w_gu[0].numel() * 2)
    tot += timed("down + residual (K=14336)", lambda i: K.decode_linear(act, w_d[i], residual=x), w_d[0].numel() * 2)
    print(f"sum of the five per layer: {tot:.1f} us -> x32 layers = {tot * 32 / 1e3:.2f} ms/token (+ lm_head, embedding, select)")
lib().mm_set_option(b"gemv_nt", 0)
# the same five launches on the MXFP8 copies (attention reads no weights: repeated for the sum only)
p_qkv, p_o, p_gu, p_d = ([K.quant_mxfp8(w) for w in ws] for ws in (w_qkv, w_o, w_gu, w_d))
for nt in (0, 1):
    lib().mm_set_option(b"gemv_nt", nt)
    print(f"-- MXFP8 weights, loads: {'non-temporal' if nt else 'default policy'}")
    tot = 0.0
    tot += timed("w8 norm + q|k|v + RoPE + append", lambda i: K.decode_qkv_rope_append_w8(x, p_qkv[i], None, Hq, Hkv, D, cos, sin, kc[i], vc[i], S, norm_w=nw, eps=1e-5), p_qkv[0].numel())
    tot += timed("attention partial+merge (S=2048)", lambda i: K.attn_decode(q, kc[i][:, :S], vc[i][:, :S], None, D ** -0.5), 2 * B * S * Hkv * D * 2)
    tot += timed("w8 o_proj + residual", lambda i: K.decode_linear_w8(x, p_o[i], H, residual=x), p_o[0].numel())
    tot += timed("w8 norm + gate|up + SwiGLU", lambda i: K.decode_gateup_swiglu_w8(x, p_gu[i], I, norm_w=nw, eps=1e-5), p_gu[0].numel())
    tot += timed("w8 down + residual (K=14336)", lambda i: K.decode_linear_w8(act, p_d[i], H, residual=x), p_d[0].numel())
    print(f"sum of the five per layer: {tot:.1f} us -> x32 layers = {tot * 32 / 1e3:.2f} ms/token (+ lm_head, embedding, select)")
lib().mm_set_option(b"gemv_nt", 0)
del p_qkv, p_o, p_gu, p_d
# the KV cache in bf16 and in MXFP8: the attention launch over S keys, and what an MXFP8 step adds (the quantising append of one position)
print("-- KV cache: bf16 and MXFP8")
Smax = S + 8
c8 = [K.kv8_append(kc[i], vc[i], torch.empty(K.kv8_bytes(B, Smax, Hkv, D), dtype=torch.uint8, device=dev), Smax, 0) for i in range(L)]
k1, v1 = torch.randn(B, 1, Hkv, D, device=dev, dtype=bf), torch.randn(B, 1, Hkv, D, device=dev, dtype=bf)
timed(f"attention, bf16 cache (S={S})", lambda i: K.attn_decode(q, kc[i][:, :S], vc[i][:, :S], None, D ** -0.5), 2 * B * S * Hkv * D * 2)
timed(f"attention, MXFP8 cache (S={S})", lambda i: K.attn_decode_kv8(q, c8[i], S, Smax, Hkv, None, D ** -0.5), 2 * B * S * Hkv * (D + D // 32))
timed("MXFP8 append of one position (S=1)", lambda i: K.kv8_append(k1, v1, c8[i], Smax, S), 2 * B * Hkv * (D * 2 + D + D // 32))
del c8
for wgs in (1, 2, 3):
    lib().mm_set_option(b"gemv_wgs", wgs)
    print(f"-- persistent workgroups per CU: {wgs}")
    timed("norm + q|k|v + RoPE + append", lambda i: K.decode_qkv_rope_append(x, w_qkv[i], None, Hq, Hkv, D, cos, sin, kc[i], vc[i], S, norm_w=nw, eps=1e-5), w_qkv[0].numel() * 2)
    timed("norm + gate|up + SwiGLU", lambda i: K.decode_gateup_swiglu(x, w_gu[i], I, norm_w=nw, eps=1e-5), w_gu[0].numel() * 2)
    timed("down + residual", lambda i: K.decode_linear(act, w_d[i], residual=x), w_d[0].numel() * 2)
lib().mm_set_option(b"gemv_wgs", 0)
for wgs in (256, 512, 768, 1024, 1536):
    lib().mm_set_option(b"attn_decode_wgs", wgs)
    timed(f"attention, ~{wgs} workgroups", lambda i: K.attn_decode(q, kc[i][:, :S], vc[i][:, :S], None, D ** -0.5), 2 * B * S * Hkv * D * 2)
lib().mm_set_option(b"attn_decode_wgs", 768)
lib().mm_set_option(b"attn_decode_mfma", 0)
timed("attention, scores on the vector ALU (round-2 slice kernel)", lambda i: K.attn_decode(q, kc[i][:, :S], vc[i][:, :S], None, D ** -0.5), 2 * B * S * Hkv * D * 2)
lib().mm_set_option(b"attn_decode_mfma", 1)
lib().mm_set_option(b"gemv_stream", 0)
timed("round-2 kernel: plain o_proj", lambda i: K.linear_fwd(x, w_o[i]), w_o[0].numel() * 2)
timed("round-2 kernel: plain down", lambda i: K.linear_fwd(act, w_d[i]), w_d[0].numel() * 2)
timed("round-2 kernel: plain gate|up", lambda i: K.linear_fwd(x, w_gu[i]), w_gu[0].numel() * 2)
lib().mm_set_option(b"gemv_stream", 1)
