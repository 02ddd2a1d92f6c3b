#!/usr/bin/env python3
"""Attention micro-benchmark at the 8B step's shape (B=4,S=2048,Hq=32,Hkv=8,D=128 causal) + ViT shape."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from multimeditron_amd import kernels as K


def run(B, S, Hq, Hkv, D, causal, mask=False):
    W = (Hq + 2 * Hkv) * D
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(B * S, W, device="cuda", generator=g).to(torch.bfloat16)
    q = qkv[:, : Hq * D].view(B, S, Hq, D); k = qkv[:, Hq * D:(Hq + Hkv) * D].view(B, S, Hkv, D); v = qkv[:, (Hq + Hkv) * D:].view(B, S, Hkv, D)
    dqkv = torch.empty_like(qkv)
    dq = dqkv[:, : Hq * D].view(B, S, Hq, D); dk = dqkv[:, Hq * D:(Hq + Hkv) * D].view(B, S, Hkv, D); dv = dqkv[:, (Hq + Hkv) * D:].view(B, S, Hkv, D)
    do = torch.randn(B, S, Hq, D, device="cuda", generator=g).to(torch.bfloat16)
    sc = D ** -0.5
    km = torch.ones(B, S, dtype=torch.long, device="cuda") if mask else None     # all-ones key mask, as the collator sends
    out, lse = K.attn_fwd(q, k, v, km, causal, sc)
    K.attn_bwd(q, k, v, out, do, lse, km, causal, sc, dq, dk, dv)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    it = 5
    ev[0].record()
    for _ in range(it):
        out, lse = K.attn_fwd(q, k, v, km, causal, sc)
    ev[1].record()
    for _ in range(it):
        K.attn_bwd(q, k, v, out, do, lse, km, causal, sc, dq, dk, dv)
    ev[2].record()
    torch.cuda.synchronize()
    f = 4.0 * B * Hq * S * S * D * (0.5 if causal else 1.0)
    tf, tb = ev[0].elapsed_time(ev[1]) / it, ev[1].elapsed_time(ev[2]) / it
    print(f"B={B} S={S} Hq={Hq} Hkv={Hkv} D={D} causal={causal} mask={mask}: fwd {tf:.3f} ms ({f / tf / 1e9:.0f} TF/s)  bwd {tb:.3f} ms ({2.5 * f / tb / 1e9:.0f} TF/s algorithmic)", flush=True)


from multimeditron_amd._lib import lib as _rawlib


class _Checked:
    """mm_set_option with its return code checked (an unknown switch means the library is older than this script)."""
    def mm_set_option(self, name, value):
        rc = _rawlib().mm_set_option(name, value)
        assert rc == 0, (name, value, rc)
        return rc


def lib():
    return _Checked()


if "--diag-q" in sys.argv:       # timing experiments on the out-of-phase forward (wrong results by design)
    lib().mm_set_option(b"attn_q_prio", 1)
    run(4, 2048, 32, 8, 128, True)
    for d in (0, 1, 2, 4, 8, 16, 4 | 8, 2 | 16, 1 | 16, 1 | 2 | 16, 4 | 8 | 16 | 1, 0):
        lib().mm_set_option(b"attn_diag", d)
        print("diag", d)
        run(4, 2048, 32, 8, 128, True)
    sys.exit(0)
if "--quick" in sys.argv:
    run(4, 2048, 32, 8, 128, True)
    run(4, 2048, 32, 8, 128, True)
    run(4, 2048, 32, 8, 128, True, mask=True)
    run(4, 2048, 32, 8, 128, True, mask=True)
    sys.exit(0)
run(4, 2048, 32, 8, 128, True)
run(4, 2048, 32, 8, 128, True)
run(4, 257, 16, 16, 64, False)
run(2, 4096, 32, 8, 128, True)
