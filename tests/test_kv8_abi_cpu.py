"""The MXFP8 KV-cache entry points (CPU): declared by the header, exported by the library, the size of the buffer they promise,
refusing what they cannot run before any launch (no device is asked for, no pointer is dereferenced), the slice length of
mm_attn_decode_kv8, and the build's resource remarks of the new kernel instantiations: no scratch."""
import ctypes
import os
import re

import pytest

from multimeditron_amd import _lib

BUILD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multimeditron_amd", "csrc", "build")
NEW = ("mm_kv8_bytes", "mm_kv8_append", "mm_kv8_dequant", "mm_attn_decode_kv8_chunk", "mm_attn_decode_kv8")
UNSUPPORTED, ARG, ALIGN = -3, -1, -2
BF16, F32 = 0, 1


def test_symbols_declared_and_exported():
    protos = _lib.parse_header()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in protos, f"include/mm_hip.h does not declare {name}"
        assert hasattr(L, name), f"libmmhip.so does not export {name}"
    assert protos["mm_kv8_bytes"][0] is ctypes.c_int64
    assert len(protos["mm_kv8_append"][1]) == 15 and len(protos["mm_kv8_dequant"][1]) == 12
    assert len(protos["mm_attn_decode_kv8"][1]) == 17 and len(protos["mm_attn_decode_kv8_chunk"][1]) == 2


@pytest.mark.parametrize("B,Smax,Hkv", [(1, 1, 1), (3, 77, 2), (16, 4129, 8)])
def test_buffer_size_is_the_memory_claim(B, Smax, Hkv):
    n = _lib.lib().mm_kv8_bytes(B, Smax, Hkv, 128)
    assert n % 16 == 0
    assert 2 * B * Smax * Hkv * 132 <= n <= 2 * B * ((Smax + 15) // 16 * 16) * Hkv * 132 + 64


def test_buffer_size_refusals():
    L = _lib.lib()
    assert L.mm_kv8_bytes(2, 16, 2, 64) == UNSUPPORTED
    for args in ((0, 16, 2, 128), (2, 0, 2, 128), (2, 16, 0, 128), (2, 16, 2, 0), (-1, 16, 2, 128)):
        assert L.mm_kv8_bytes(*args) == ARG, args


def test_refusals_come_before_any_launch():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    W = 4 * 128                                    # a fused q|k|v row of (2 + 1 + 1) heads

    def append(dtype=BF16, k=p, v=p, B=2, S=3, Hkv=1, D=128, ksb=3 * W, kss=W, vsb=3 * W, vss=W, cache=p, Smax=8, pos=0):
        return L.mm_kv8_append(dtype, k, v, B, S, Hkv, D, ksb, kss, vsb, vss, cache, Smax, pos, None)

    def dequant(cache=p, B=2, Smax=8, Hkv=1, D=128, pos=0, S=3, ko=p, vo=p, sb=3 * 128, ss=128):
        return L.mm_kv8_dequant(cache, B, Smax, Hkv, D, pos, S, ko, vo, sb, ss, None)

    def attn(dtype=BF16, q=p, cache=p, B=2, Skv=5, Smax=8, Hq=2, Hkv=1, D=128, qsb=W, qsh=128, mask=None, out=p, ws=p, ns=1):
        return L.mm_attn_decode_kv8(dtype, q, cache, B, Skv, Smax, Hq, Hkv, D, qsb, qsh, mask, ctypes.c_float(0.1), out, ws, ns, None)

    # D = 64
    assert append(D=64) == UNSUPPORTED and dequant(D=64) == UNSUPPORTED and attn(D=64) == UNSUPPORTED
    # fp32
    assert append(dtype=F32) == UNSUPPORTED and attn(dtype=F32) == UNSUPPORTED
    # Hq / Hkv = 8 (and 7): outside the MFMA slice kernel's range
    assert attn(Hq=8, Hkv=1) == UNSUPPORTED and attn(Hq=7, Hkv=1) == UNSUPPORTED
    assert attn(Hq=3, Hkv=2) == ARG
    # pos + S > Smax
    assert append(pos=6) == ARG and append(S=9) == ARG and append(pos=-1) == ARG
    assert dequant(pos=6) == ARG
    assert attn(Skv=9) == ARG and attn(Skv=0) == ARG and attn(ns=0) == ARG
    # NULL operands
    for name in ("k", "v", "cache"):
        assert append(**{name: None}) == ARG, name
    for name in ("cache", "ko", "vo"):
        assert dequant(**{name: None}) == ARG, name
    for name in ("q", "cache", "out", "ws"):
        assert attn(**{name: None}) == ARG, name
    # a misaligned q / source / buffer
    assert attn(q=p + 8) == ALIGN and attn(cache=p + 4) == ALIGN
    assert append(k=p + 2) == ALIGN and append(v=p + 8) == ALIGN and append(cache=p + 8) == ALIGN
    # a stride that is not a multiple of 8
    assert append(kss=W + 4) == ALIGN and append(vsb=3 * W + 2) == ALIGN
    assert dequant(ss=132) == ALIGN
    assert attn(qsb=W + 4) == ALIGN and attn(qsh=130) == ALIGN


def test_slice_length():
    L = _lib.lib()
    assert L.mm_attn_decode_kv8_chunk(0, 1) == ARG and L.mm_attn_decode_kv8_chunk(5, 0) == ARG
    A = L.mm_attn_decode_kv8_chunk(1, 1)                     # one key: the alignment itself
    assert A & (A - 1) == 0 and 1 <= A <= 16
    for Skv in (1, 2, 15, 16, 17, 63, 64, 65, 130, 777, 2049, 4129, 131072):
        for ns in (1, 2, 3, 5, 13, 24, 96, 768):
            c = L.mm_attn_decode_kv8_chunk(Skv, ns)
            need = -(-Skv // ns)
            assert c % A == 0 and need <= c < need + A and ns * c >= Skv, (Skv, ns, c)


def _remarks(path):
    out, cur = {}, None
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and cur is not None:
            cur["scratch"] = int(m.group(1))
    return out


def test_new_kernels_use_no_scratch():
    paths = [os.path.join(BUILD, f) for f in ("mm_attn.o.resources.txt", "mm_kv8.o.resources.txt")]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("library not built in this tree (python multimeditron_amd/csrc/build.py)")
    attn, kv8 = (_remarks(p) for p in paths)
    mfma = {n: r for n, r in attn.items() if "attn_decode_partial128_mfma_kernel" in n}
    # G in {1, 2, 4} in both cache formats (the last template argument: Lb0E bf16, Lb1E MXFP8)
    assert len(mfma) == 6 and sum(1 for n in mfma if "Lb1EEEv" in n) == 3, sorted(mfma)
    new = {n: r for n, r in mfma.items() if "Lb1EEEv" in n}
    new.update({n: r for n, r in kv8.items() if "kv8_append_kernel" in n or "kv8_dequant_kernel" in n})
    assert len(new) == 5, sorted(new)
    for name, r in sorted(new.items()):
        assert r["scratch"] == 0, f"{name}: {r['scratch']} bytes/lane of scratch"
