"""Kernel contract of Qwen3's fused per-head q/k RMSNorm + RoPE (include/mm_hip.h, csrc/mm_qknorm.hip).

Forward: given the kernel's own rstd, the output must be BIT-identical to the documented rounding chain -- bf16(x * rstd) (one
fp32 product, one rounding), bf16(w * that) (a product of two bf16 values, exact in fp32, one rounding), then mm_rope_apply with
the same tables -- taken here in torch + the existing mm_rope_apply.  Against mm_rmsnorm_fwd on a contiguous [T*H, D] copy +
mm_rope_apply: bit-identical on every head whose rstd agrees, last-bit differences on the others only.  rstd against fp64.
Backward: per-element fp64 bounds |got - ref| <= c u E (tests/kernel_check.check_bound) with E built from absolute terms; dx lands in
a NaN-sentinel storage (kernel_check.Guarded) that also holds the v columns and row padding, which must stay untouched.  The dw
partials are bit-identical across reruns.  Decode: the append kernel is bit-identical to the forward in place + the cache copy."""
import ctypes
import os
import re

import pytest
import torch

from tests.kernel_check import U, U32, Guarded, check_bound

BF = torch.bfloat16
EPS = 1e-6
BUILD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multimeditron_amd", "csrc", "build")
C_BWD = 2.0          # err / (u E) of dx and dw

HEADS = [(32, 8), (4, 1), (16, 8)]
TOKENS = [1, 7, 8195]


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def problem(dtype, D, Hq, Hkv, T, seed, pad=16):
    """qkv [T, (Hq+2Hkv)*D + pad] (row stride wider than the projection), per-(token, head) scales so rstd varies, norm weights
    around 1, Qwen3's default RoPE tables (theta 1e6) at positions 3..T+2."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    nh, W = Hq + Hkv, (Hq + 2 * Hkv) * D
    scale = (0.1 + 2.0 * torch.rand(T, Hq + 2 * Hkv, 1, generator=g, device="cuda")).expand(T, Hq + 2 * Hkv, D).reshape(T, W)
    qkv = torch.randn(T, W + pad, generator=g, device="cuda")
    qkv[:, :W] *= scale
    qkv = qkv.to(dtype)
    wq = (1.0 + 0.1 * torch.randn(D, generator=g, device="cuda")).to(dtype)
    wk = (1.0 + 0.1 * torch.randn(D, generator=g, device="cuda")).to(dtype)
    from multimeditron_amd import kernels as K
    pos = torch.arange(3, T + 3, device="cuda", dtype=torch.int64)
    inv = 1.0 / (1e6 ** (torch.arange(0, D, 2, device="cuda", dtype=torch.int64).float() / D))
    cos, sin = K.rope_table(pos, inv, dtype == BF)
    return qkv, wq, wk, cos, sin


def head_weights(wq, wk, Hq, Hkv):
    D = wq.numel()
    return torch.cat([wq.float().expand(Hq, D), wk.float().expand(Hkv, D)]).unsqueeze(0)        # [1, nh, D]


def chain_reference(qkv, rstd, wq, wk, cos, sin, T, Hq, Hkv, D):
    """The documented rounding chain on the kernel's own rstd, then the existing mm_rope_apply."""
    from multimeditron_amd import kernels as K
    nh = Hq + Hkv
    x = qkv[:, : nh * D].reshape(T, nh, D).float()
    n = (x * rstd.view(T, nh, 1)).to(qkv.dtype).float()
    y = (head_weights(wq, wk, Hq, Hkv) * n).to(qkv.dtype).reshape(T, nh * D).contiguous()
    K.rope_apply_(y, T, nh, D, nh * D, cos, sin)
    return y


def rstd64(qkv, T, nh, D):
    x = qkv[:, : nh * D].reshape(T, nh, D).double()
    return 1.0 / torch.sqrt((x * x).mean(-1) + EPS)


@pytest.mark.gpu
@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_forward_exact_chain_and_rmsnorm_composition(dtype, D, Hq, Hkv, T):
    _gpu()
    from multimeditron_amd import kernels as K
    nh = Hq + Hkv
    qkv, wq, wk, cos, sin = problem(dtype, D, Hq, Hkv, T, seed=T * 7 + D + Hq)
    before = qkv.clone()
    ld_out = nh * D + 8
    gout = Guarded(T * ld_out, dtype, "cuda")
    out = gout.view((T, nh * D), (ld_out, 1))
    _, rstd = K.qk_norm_rope_fwd(qkv, T, Hq, Hkv, D, wq, wk, EPS, cos, sin, out=out)
    torch.cuda.synchronize()
    gout.verify("qk")                                          # wrote exactly the q|k heads, no row padding
    assert torch.equal(qkv.view(torch.int16 if dtype == BF else torch.int32), before.view(torch.int16 if dtype == BF else torch.int32))
    # (1) bit-identical to the rounding chain on the kernel's own rstd
    ref = chain_reference(qkv, rstd, wq, wk, cos, sin, T, Hq, Hkv, D)
    assert torch.equal(out, ref), float((out.float() - ref.float()).abs().max())
    # (2) rstd against fp64: a few fp32 ulps
    r64 = rstd64(qkv, T, nh, D)
    rel = ((rstd.double() - r64).abs() / r64).max().item()
    assert rel <= 16 * U32, rel
    # (3) mm_rmsnorm_fwd on contiguous [T*H, D] copies + mm_rope_apply: equal wherever rstd is equal, last bits elsewhere
    yq, rq = K.rmsnorm_fwd(qkv[:, : Hq * D].reshape(T * Hq, D).contiguous(), wq, EPS)
    yk, rk = K.rmsnorm_fwd(qkv[:, Hq * D: nh * D].reshape(T * Hkv, D).contiguous(), wk, EPS)
    comp = torch.cat([yq.view(T, Hq * D), yk.view(T, Hkv * D)], 1).contiguous()
    K.rope_apply_(comp, T, nh, D, nh * D, cos, sin)
    rcomp = torch.cat([rq.view(T, Hq), rk.view(T, Hkv)], 1)
    same = (rcomp == rstd).view(T, nh, 1).expand(T, nh, D)
    o3, c3 = out.reshape(T, nh, D), comp.view(T, nh, D)
    assert torch.equal(o3[same], c3[same])
    assert (((rcomp.double() - rstd.double()).abs() / r64).max().item()) <= 16 * U32
    if bool((~same).any()):
        headmax = c3.float().abs().amax(-1, keepdim=True).expand(T, nh, D)
        lastbits = (2.0 ** -6) if dtype == BF else (2.0 ** -20)
        diff = (o3.float() - c3.float()).abs()
        assert bool((diff[~same] <= lastbits * headmax[~same]).all()), float(diff[~same].max())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF, torch.float32])
@pytest.mark.parametrize("D", [128, 64])
def test_forward_in_place_equals_out_of_place(dtype, D):
    _gpu()
    from multimeditron_amd import kernels as K
    Hq, Hkv, T = 16, 8, 300
    nh, W = Hq + Hkv, (Hq + 2 * Hkv) * D
    qkv, wq, wk, cos, sin = problem(dtype, D, Hq, Hkv, T, seed=5)
    qk, rstd = K.qk_norm_rope_fwd(qkv, T, Hq, Hkv, D, wq, wk, EPS, cos, sin)
    x = qkv.clone()
    K.qk_norm_rope_fwd(x, T, Hq, Hkv, D, wq, wk, EPS, cos, sin, out=x, want_rstd=False)
    torch.cuda.synchronize()
    assert torch.equal(x[:, : nh * D], qk)
    assert torch.equal(x[:, nh * D:], qkv[:, nh * D:])          # v and the row padding untouched


def backward_reference(qkv, dqk, wq, wk, cos, sin, T, Hq, Hkv, D):
    """fp64: inverse RoPE, RMSNorm backward per head.  -> (dx, E_dx_function, dwq, dwk, sum|terms| of dwq, dwk)."""
    nh, half = Hq + Hkv, D // 2
    x = qkv[:, : nh * D].reshape(T, nh, D).double()
    d = dqk.reshape(T, nh, D).double()
    c, s = cos.double().view(T, 1, half), sin.double().view(T, 1, half)
    dl, dh = d[..., :half], d[..., half:]
    g = torch.cat([dl * c + dh * s, dh * c - dl * s], -1)
    G = torch.cat([dl.abs() * c.abs() + dh.abs() * s.abs(), dh.abs() * c.abs() + dl.abs() * s.abs()], -1)
    r = rstd64(qkv, T, nh, D).unsqueeze(-1)
    w = head_weights(wq, wk, Hq, Hkv).double()
    xh, XH = x * r, x.abs() * r
    gw, GW = g * w, G * w.abs()
    dot, DOT = (gw * xh).mean(-1, keepdim=True), (GW * XH).mean(-1, keepdim=True)
    dx = r * (gw - xh * dot)
    Ef = r * (GW + XH * DOT)
    t, T_ = g * xh, G * XH
    return (dx.reshape(T, nh * D), Ef.reshape(T, nh * D), t[:, :Hq].sum((0, 1)), t[:, Hq:].sum((0, 1)), T_[:, :Hq].sum((0, 1)),
            T_[:, Hq:].sum((0, 1)))


@pytest.mark.gpu
@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_backward_fp64_bounds_and_determinism(dtype, D, Hq, Hkv, T):
    _gpu()
    from multimeditron_amd import kernels as K
    nh, W = Hq + Hkv, (Hq + 2 * Hkv) * D
    qkv, wq, wk, cos, sin = problem(dtype, D, Hq, Hkv, T, seed=T * 3 + D + Hkv)
    _, rstd = K.qk_norm_rope_fwd(qkv, T, Hq, Hkv, D, wq, wk, EPS, cos, sin)
    g = torch.Generator(device="cuda").manual_seed(T + 11)
    dqk = torch.randn(T, nh * D, generator=g, device="cuda").to(dtype)
    ld_dx = W + 8
    gdx = Guarded(T * ld_dx, dtype, "cuda")
    dx = gdx.view((T, nh * D), (ld_dx, 1))                    # the q|k columns of dqkv; v columns + padding stay sentinel
    dwq, dwk = K.qk_norm_rope_bwd(dqk, qkv, T, Hq, Hkv, D, wq, wk, rstd, cos, sin, dx)
    torch.cuda.synchronize()
    gdx.verify("dqkv")
    u = U[dtype]
    ref, Ef, rq, rk, Sq, Sk = backward_reference(qkv, dqk, wq, wk, cos, sin, T, Hq, Hkv, D)
    check_bound("dx", dx, ref, ref.abs() + (D + 16) * (U32 / u) * Ef, C_BWD, u=u)
    nblk = K.qk_norm_bwd_blocks(T)
    assert dwq.shape == (nblk, D) and dwk.shape == (nblk, D)
    depth = 8 * nh + nblk + 128                               # longest fp32 summation chain (lane, LDS, reduce_partials)
    for name, part, r_, S_ in (("dw_q", dwq, rq, Sq), ("dw_k", dwk, rk, Sk)):
        out = torch.empty(D, dtype=torch.float32, device="cuda")
        K.reduce_partials(part, out, False)
        check_bound(name, out, r_, r_.abs() + depth * S_, C_BWD, u=U32)
    # deterministic: a rerun is bit-identical; without partials dx is unchanged
    dx2 = torch.empty(T, W, dtype=dtype, device="cuda")
    dwq2, dwk2 = K.qk_norm_rope_bwd(dqk, qkv, T, Hq, Hkv, D, wq, wk, rstd, cos, sin, dx2)
    dx3 = torch.empty(T, W, dtype=dtype, device="cuda")
    none = K.qk_norm_rope_bwd(dqk, qkv, T, Hq, Hkv, D, wq, wk, rstd, cos, sin, dx3, want_dw=False)
    torch.cuda.synchronize()
    assert none == (None, None)
    assert torch.equal(dwq2, dwq) and torch.equal(dwk2, dwk)
    assert torch.equal(dx2[:, : nh * D], dx) and torch.equal(dx3[:, : nh * D], dx)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF, torch.float32])
@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_append_equals_forward_plus_cache_copy(dtype, D, Hq, Hkv):
    _gpu()
    from multimeditron_amd import kernels as K
    B, Smax, pos = 7, 12, 5
    nh, W = Hq + Hkv, (Hq + 2 * Hkv) * D
    qkv, wq, wk, cos, sin = problem(dtype, D, Hq, Hkv, B, seed=D + Hq)
    qkv = qkv[:, :W].contiguous()
    kc = torch.zeros(B, Smax, Hkv, D, dtype=dtype, device="cuda")
    vc = torch.zeros_like(kc)
    a = qkv.clone()
    K.qk_norm_rope_append_(a, B, Hq, Hkv, D, wq, wk, EPS, cos, sin, kc, vc, pos)
    f = qkv.clone()
    K.qk_norm_rope_fwd(f, B, Hq, Hkv, D, wq, wk, EPS, cos, sin, out=f, want_rstd=False)
    torch.cuda.synchronize()
    assert torch.equal(a, f)
    assert torch.equal(kc[:, pos].reshape(B, Hkv * D), f[:, Hq * D: nh * D])
    assert torch.equal(vc[:, pos].reshape(B, Hkv * D), qkv[:, nh * D:])
    others = torch.ones(Smax, dtype=torch.bool)
    others[pos] = False
    assert not bool(kc[:, others].any()) and not bool(vc[:, others].any())


@pytest.mark.gpu
def test_other_head_widths_are_unsupported():
    _gpu()
    from multimeditron_amd import _lib
    L = _lib.lib()
    D, Hq, Hkv, T = 96, 4, 1, 8
    x = torch.zeros(T, (Hq + 2 * Hkv) * D, dtype=BF, device="cuda")
    w = torch.ones(D, dtype=BF, device="cuda")
    cs = torch.zeros(T, D // 2, device="cuda")
    r = torch.empty(T, Hq + Hkv, device="cuda")
    kc = torch.zeros(T, 4, Hkv, D, dtype=BF, device="cuda")
    W, p = x.shape[1], x.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    UNSUPPORTED = -3
    assert L.mm_qk_norm_rope_fwd(_lib.MM_BF16, p, W, T, Hq, Hkv, D, w.data_ptr(), w.data_ptr(), ctypes.c_float(EPS), cs.data_ptr(),
                                 cs.data_ptr(), p, W, r.data_ptr(), s) == UNSUPPORTED
    assert L.mm_qk_norm_rope_bwd(_lib.MM_BF16, p, W, p, W, T, Hq, Hkv, D, w.data_ptr(), w.data_ptr(), r.data_ptr(), cs.data_ptr(),
                                 cs.data_ptr(), p, W, None, None, s) == UNSUPPORTED
    assert L.mm_qk_norm_rope_append(_lib.MM_BF16, p, T, Hq, Hkv, D, W, w.data_ptr(), w.data_ptr(), ctypes.c_float(EPS), cs.data_ptr(),
                                    cs.data_ptr(), kc.data_ptr(), kc.data_ptr(), 4 * Hkv * D, s) == UNSUPPORTED
    assert "unsupported" in L.mm_error_string(UNSUPPORTED).decode()


def test_qk_norm_kernels_use_no_scratch():
    """The three kernels keep everything in registers (and the backward's 16-32 KB of LDS)."""
    path = os.path.join(BUILD, "mm_qknorm.o.resources.txt")
    if not os.path.exists(path):
        pytest.skip("library not built in this tree (python multimeditron_amd/csrc/build.py)")
    seen, name = {}, None
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and name:
            for k in ("qk_norm_rope_fwd_kernel", "qk_norm_rope_bwd_kernel", "qk_norm_rope_append_kernel"):
                if k in name:
                    seen.setdefault(k, []).append(int(m.group(1)))
    assert sorted(seen) == ["qk_norm_rope_append_kernel", "qk_norm_rope_bwd_kernel", "qk_norm_rope_fwd_kernel"], seen
    for k, v in seen.items():
        assert len(v) == 4 and all(x == 0 for x in v), (k, v)           # bf16 / f32 x D = 64 / 128
