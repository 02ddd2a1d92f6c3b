"""The shared-prefix decode attention entry points (CPU): declared by the header, exported by the library, refusing what they cannot
run before any launch (no device is asked for, no pointer is dereferenced), the split count under attn_decode_wgs = 1, and the
build's resource remarks of the new kernel instantiations: no scratch."""
import ctypes
import os
import re

import pytest

from multimeditron_amd import _lib

BUILD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multimeditron_amd", "csrc", "build")
NEW = ("mm_attn_decode_shared_splits", "mm_attn_decode_shared")
UNSUPPORTED, ARG, ALIGN = -3, -1, -2
BF16, F32 = 0, 1


def test_symbols_declared_and_exported():
    protos = _lib.parse_header()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in protos, f"include/mm_hip.h does not declare {name}"
        assert hasattr(L, name), f"libmmhip.so does not export {name}"
    assert len(protos["mm_attn_decode_shared_splits"][1]) == 4 and len(protos["mm_attn_decode_shared"][1]) == 33


def test_refusals_come_before_any_launch():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    W = 4 * 128                                    # a fused q|k|v row of (2 + 1 + 1) heads
    STRIDES = ("qsb", "qsh", "kpsb", "kpss", "kpsh", "vpsb", "vpss", "vpsh", "kssb", "ksss", "kssh", "vssb", "vsss", "vssh")

    def attn(dtype=BF16, q=p, kp=p, vp=p, ks=p, vs=p, B=2, n=3, Sp=5, Ss=2, Hq=2, Hkv=1, D=128, mask=None, out=p, ws=p, ns=1, **st):
        s = dict(qsb=W, qsh=128, kpsb=8 * 128, kpss=128, kpsh=128, vpsb=8 * 128, vpss=128, vpsh=128, kssb=4 * 128, ksss=128, kssh=128,
                 vssb=4 * 128, vsss=128, vssh=128)
        assert set(st) <= set(s)
        s.update(st)
        return L.mm_attn_decode_shared(dtype, q, kp, vp, ks, vs, B, n, Sp, Ss, Hq, Hkv, D, *(s[k] for k in STRIDES), mask,
                                       ctypes.c_float(0.1), out, ws, ns, None)

    # D = 64, fp32
    assert attn(D=64) == UNSUPPORTED and attn(dtype=F32) == UNSUPPORTED
    # Hq / Hkv = 7 and 8: more than the column tile is written for
    assert attn(Hq=8, Hkv=1) == UNSUPPORTED and attn(Hq=7, Hkv=1) == UNSUPPORTED
    assert attn(Hq=3, Hkv=2) == ARG
    # sizes
    assert attn(Sp=0) == ARG and attn(Ss=0) == ARG and attn(n=0) == ARG and attn(ns=0) == ARG and attn(B=-1) == ARG
    # NULL operands
    for name in ("q", "kp", "vp", "ks", "vs", "out", "ws"):
        assert attn(**{name: None}) == ARG, name
    # misaligned pointers
    for name in ("q", "kp", "vp", "ks", "vs"):
        assert attn(**{name: p + 8}) == ALIGN, name
    # a stride that is not a multiple of 8
    for name in STRIDES:
        assert attn(**{name: 132}) == ALIGN, name
    # the shape checks come first: a refused shape with a bad stride is still the shape's code
    assert attn(D=64, qsb=W + 4) == UNSUPPORTED and attn(n=0, q=p + 8) == ARG


def test_split_count():
    L = _lib.lib()
    old = ctypes.c_int(0)
    assert L.mm_get_option(b"attn_decode_wgs", ctypes.byref(old)) == 0
    try:
        assert L.mm_set_option(b"attn_decode_wgs", 1) == 0
        for B, n, Hkv, Skv in ((1, 1, 1, 1), (4, 4, 8, 2081), (2, 3, 1, 150), (3, 9, 2, 4129)):
            assert L.mm_attn_decode_shared_splits(B, n, Hkv, Skv) == 1, (B, n, Hkv, Skv)
        assert L.mm_set_option(b"attn_decode_wgs", 768) == 0
        # ceil(2 * 768 / 3) = 512 workgroups over B * ceil(n / 4) * Hkv per slice, at least 64 keys per slice, at least one slice
        assert L.mm_attn_decode_shared_splits(4, 4, 8, 2081) == 16             # 512 / 32
        assert L.mm_attn_decode_shared_splits(4, 5, 8, 2081) == 8              # two tiles: 512 / 64
        assert L.mm_attn_decode_shared_splits(1, 1, 1, 130) == 3               # capped by the keys
        assert L.mm_attn_decode_shared_splits(16, 64, 8, 4096) == 1
        assert L.mm_attn_decode_shared_splits(0, 4, 8, 100) == 1 and L.mm_attn_decode_shared_splits(4, 0, 8, 100) == 1
        from tests.attn_shared_check import shared_splits
        for wgs in (8, 100, 768, 1536):
            assert L.mm_set_option(b"attn_decode_wgs", wgs) == 0
            for B, n, Hkv, Skv in ((1, 1, 1, 77), (4, 4, 8, 2048), (3, 9, 2, 4129), (2, 17, 1, 700)):
                assert L.mm_attn_decode_shared_splits(B, n, Hkv, Skv) == shared_splits(B, n, Hkv, Skv, wgs), (wgs, B, n, Hkv, Skv)
    finally:
        assert L.mm_set_option(b"attn_decode_wgs", old.value) == 0


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
    path = os.path.join(BUILD, "mm_attn.o.resources.txt")
    if not os.path.exists(path):
        pytest.skip("library not built in this tree (python multimeditron_amd/csrc/build.py)")
    new = {n: r for n, r in _remarks(path).items() if "attn_decode_shared128_kernel" in n}
    assert len(new) == 3, sorted(new)                       # G in {1, 2, 4}
    for name, r in sorted(new.items()):
        assert r["scratch"] == 0, f"{name}: {r['scratch']} bytes/lane of scratch"
