"""The MXFP8 KV cache through the C ABI (include/mm_hip.h: mm_kv8_append, mm_kv8_dequant, mm_attn_decode_kv8), held to exact results
wherever the contract promises them.

Append / dequant: the rows a buffer stands for are tests/w8_check.roundtrip_ref of the rows appended, bit for bit (the format is
mm_quant_mxfp8's, restated there), and nothing outside the appended positions changes.
Attention: whenever the slices coincide the output has the bits of mm_attn_decode (tests/attn_check.run_decode) on the dequantised
rows; under every other slicing it is held to the fp64 reference of the DEQUANTISED operands with the constant the MFMA decode
kernel is held to (the arithmetic is the same), and the two exact families hold bitwise.  Every attention case runs on a buffer
pre-filled with zeros and on one pre-filled with 0xFF bytes (NaN elements, NaN scales): a slot nobody appended to is never used.
Outputs, workspaces and cache buffers live in kernel_check.Guarded storages."""
import pytest
import torch

from multimeditron_amd._lib import call, lib
from tests import attn_check as A
from tests import w8_check as W8
from tests.kernel_check import Guarded, check_bits, dt, ptr, stream, verify_guards

pytestmark = pytest.mark.gpu

D = 128
BF16 = torch.bfloat16


class Cache:
    """One layer's buffer of mm_kv8_bytes inside a guarded storage, every byte pre-filled with `fill`."""

    def __init__(self, B, Smax, Hkv, fill=0):
        self.B, self.Smax, self.Hkv = B, Smax, Hkv
        n = lib().mm_kv8_bytes(B, Smax, Hkv, D)
        assert n > 0 and n % 16 == 0
        self.guard = Guarded(n // 2, BF16, "cuda")
        self.bytes = self.guard.view((n // 2,), (1,)).view(torch.uint8)
        self.bytes.fill_(fill)
        assert self.bytes.data_ptr() % 16 == 0

    def append(self, k, v, pos):
        B, S, Hkv, _ = k.shape
        call("mm_kv8_append", dt(k.dtype), ptr(k), ptr(v), B, S, Hkv, D, k.stride(0), k.stride(1), v.stride(0), v.stride(1),
             ptr(self.bytes), self.Smax, pos, stream())

    def dequant(self, pos, S):
        """-> k, v [B, S, Hkv, D] as strided views (a longer position stride) inside guarded storages, and the guards"""
        B, Hkv = self.B, self.Hkv
        ss = Hkv * D + 8
        gk, gv = (Guarded(B * S * ss, BF16, "cuda") for _ in range(2))
        k, v = (g.view((B, S, Hkv, D), (S * ss, ss, D, 1)) for g in (gk, gv))
        call("mm_kv8_dequant", ptr(self.bytes), B, self.Smax, Hkv, D, pos, S, ptr(k), ptr(v), S * ss, ss, stream())
        return k, v, [("k_out", gk), ("v_out", gv)]

    def verify(self):
        self.guard.verify("cache buffer", False)


def fused_rows(k, v, Hq):
    """k, v [B, S, Hkv, D] (CPU) -> the same rows on the device as strided views inside one q|k|v-shaped buffer [B * S, (Hq + 2 Hkv) D]"""
    B, S, Hkv, _ = k.shape
    row = torch.zeros(B * S, (Hq + 2 * Hkv) * D, dtype=BF16)
    row[:, Hq * D:(Hq + Hkv) * D] = k.reshape(B * S, Hkv * D)
    row[:, (Hq + Hkv) * D:] = v.reshape(B * S, Hkv * D)
    row = row.cuda()
    return row[:, Hq * D:(Hq + Hkv) * D].view(B, S, Hkv, D), row[:, (Hq + Hkv) * D:].view(B, S, Hkv, D)


def sample_rows(B, S, Hkv, seed):
    return W8.sample_matrix(B * S * Hkv, D, seed).view(B, S, Hkv, D)


def roundtrip(rows):
    return W8.roundtrip_ref(rows.reshape(-1, D)).view(rows.shape)


# ---- append / dequant --------------------------------------------------------------------------------------------------------------
APPEND = [(1, 1, 1, 0, 1), (3, 1, 2, 16, 40), (2, 37, 2, 0, 37), (2, 19, 8, 5, 33)]


@pytest.mark.parametrize("B,S,Hkv,pos,Smax", APPEND, ids=[f"B{c[0]}-S{c[1]}-h{c[2]}-pos{c[3]}-of{c[4]}" for c in APPEND])
def test_append_then_dequant_is_the_format_and_touches_nothing_else(B, S, Hkv, pos, Smax):
    bg_k, bg_v = sample_rows(B, Smax, Hkv, 11), sample_rows(B, Smax, Hkv, 12)
    new_k, new_v = sample_rows(B, S, Hkv, 13), sample_rows(B, S, Hkv, 14)
    c = Cache(B, Smax, Hkv, fill=0xFF)
    c.append(bg_k.cuda(), bg_v.cuda(), 0)                       # a recognisable append of every position first
    c.append(*fused_rows(new_k, new_v, 2 * Hkv), pos)
    want_k, want_v = roundtrip(bg_k), roundtrip(bg_v)
    want_k[:, pos:pos + S], want_v[:, pos:pos + S] = roundtrip(new_k), roundtrip(new_v)
    k, v, guards = c.dequant(0, Smax)
    check_bits("k of every position", k, want_k)
    check_bits("v of every position", v, want_v)
    verify_guards(guards)
    k, v, guards = c.dequant(pos, S)
    check_bits("k of the appended positions", k, want_k[:, pos:pos + S])
    check_bits("v of the appended positions", v, want_v[:, pos:pos + S])
    verify_guards(guards)
    c.verify()


def test_two_single_appends_equal_one_double_append():
    B, Hkv, Smax, pos = 3, 2, 21, 7
    k, v = sample_rows(B, 2, Hkv, 21), sample_rows(B, 2, Hkv, 22)
    kd, vd = fused_rows(k, v, 4)
    one, two = Cache(B, Smax, Hkv, fill=0x5A), Cache(B, Smax, Hkv, fill=0x5A)
    one.append(kd, vd, pos)
    two.append(kd[:, :1], vd[:, :1], pos)
    two.append(kd[:, 1:], vd[:, 1:], pos + 1)
    assert torch.equal(one.bytes, two.bytes)
    assert int((one.bytes != 0x5A).sum()) <= 2 * B * 2 * Hkv * 132          # at most the bytes of two positions changed
    one.verify(), two.verify()


# ---- attention ---------------------------------------------------------------------------------------------------------------------
HEADS = [(1, 2, 2), (3, 4, 2), (2, 4, 1), (2, 8, 2)]                        # G = 1, 2, 4, 4
COINCIDE = [(1, 1), (15, 1), (16, 1), (17, 1), (63, 1), (65, 1), (128, 2), (200, 13), (1000, 1)]
MASKS = [None, "leftpad", "holes", "dead", "single"]
FILLS = [0x00, 0xFF]


def nsplit_of(ns, B, Hkv, Skv):
    return lib().mm_attn_decode_splits(B, Hkv, Skv) if ns == "lib" else ns


def filled_cache(k, v, fill, spare=11):
    """k, v [B, Skv, Hkv, D] (CPU) appended to a buffer of Skv + spare positions pre-filled with `fill`"""
    B, Skv, Hkv, _ = k.shape
    c = Cache(B, Skv + spare, Hkv, fill)
    c.append(*fused_rows(k, v, Hkv), 0)
    return c


def run_kv8(q, c, Skv, mask, scale, ns):
    """mm_attn_decode_kv8 with out and the workspace inside guarded storages (every slice's record must be written)"""
    B, Hq, _ = q.shape
    out, ws, guards = A.decode_buffers(B, Hq, D, ns, q.device)
    call("mm_attn_decode_kv8", dt(q.dtype), ptr(q), ptr(c.bytes), B, Skv, c.Smax, Hq, c.Hkv, D, q.stride(0), q.stride(1), ptr(mask),
         float(scale), ptr(out), ptr(ws), ns, stream())
    return out, guards


@pytest.mark.parametrize("B,Hq,Hkv", HEADS, ids=[f"B{h[0]}-h{h[1]}x{h[2]}" for h in HEADS])
@pytest.mark.parametrize("Skv,ns", COINCIDE, ids=[f"k{s}-ns{n}" for s, n in COINCIDE])
def test_attention_has_the_bits_of_the_bf16_kernel_on_the_dequantised_rows(Skv, ns, B, Hq, Hkv):
    chunk = lib().mm_attn_decode_kv8_chunk(Skv, ns)
    assert ns == 1 or chunk == A.decode_chunk(Skv, ns), "not a case whose slices coincide"
    case = A.decode_case(B, Skv, Hq, Hkv, D)
    scale = D ** -0.5
    for kind in MASKS:
        m = A.decode_mask(kind, B, Skv, ns)
        q, k, v = A.decode_operands(case, m)
        qd, _, _ = A.decode_place(q, k, v)
        md = m.cuda() if m is not None else None
        want = None
        for fill in FILLS:
            c = filled_cache(k, v, fill)
            if want is None:
                kd, vd, _ = c.dequant(0, Skv)
                want, guards, _ = A.run_decode(qd, kd, vd, md, scale, nsplit=ns)
                verify_guards(guards)
            out, guards = run_kv8(qd, c, Skv, md, scale, ns)
            check_bits(f"out (mask {kind}, buffer pre-filled with {fill:#04x})", out, want)
            verify_guards(guards)
            c.verify()


SLICINGS = [(130, 3), (777, 5), (2049, "lib")]


@pytest.mark.parametrize("B,Hq,Hkv", HEADS[1:], ids=[f"B{h[0]}-h{h[1]}x{h[2]}" for h in HEADS[1:]])
@pytest.mark.parametrize("Skv,ns", SLICINGS, ids=[f"k{s}-ns{n}" for s, n in SLICINGS])
def test_attention_under_every_slicing(Skv, ns, B, Hq, Hkv, monkeypatch):
    ns = nsplit_of(ns, B, Hkv, Skv)
    # the exact families take the slice boundaries from the library
    monkeypatch.setattr(A, "decode_chunk", lambda skv, n: lib().mm_attn_decode_kv8_chunk(skv, n))
    case = A.decode_case(B, Skv, Hq, Hkv, D)
    scale = D ** -0.5
    G = Hq // Hkv

    def runs(q, k, v, m):
        qd, _, _ = A.decode_place(q, k, v)
        md = m.cuda() if m is not None else None
        outs = []
        for fill in FILLS:
            c = filled_cache(k, v, fill)
            out, guards = run_kv8(qd, c, Skv, md, scale, ns)
            verify_guards(guards)
            c.verify()
            outs.append(out)
        check_bits("out over a buffer pre-filled with 0xff against one pre-filled with zeros", outs[1], outs[0])
        kd, vd, _ = c.dequant(0, Skv)
        return outs[0], kd.cpu(), vd.cpu()

    # fp64 bound on the dequantised operands
    for kind in (None, "holes", "slice"):
        m = A.decode_mask(kind, B, Skv, ns)
        q, k, v = A.decode_operands(case, m)
        out, kd, vd = runs(q, k, v, m)
        ref = A.decode_reference(q, kd, vd, m, scale)
        worst = A.check_decode(out, ref, None, c=A.C["bf16-decode-mfma"]["out"])
        print(f"k{Skv} ns{ns} B{B} h{Hq}x{Hkv} mask {kind}: err/(u E) = {worst:.3g}")

    # one visible key per sequence: that key's dequantised V row, bit for bit
    q, k, v, m, _ = A.decode_one_key(case, ns)
    out, kd, vd = runs(q, k, v, m)
    want = torch.stack([vd[b, int(m[b].argmax())] for b in range(B)]).repeat_interleave(G, dim=1)
    check_bits("one_key", out, want)

    # q = 0 and small-integer V (exact in e4m3): the mean of the visible rows, bit for bit
    q, k, v, m, want = A.decode_uniform(case)
    out, kd, vd = runs(q, k, v, m)
    check_bits("uniform: V survives the quantiser", vd, v)
    check_bits("uniform", out, want)
