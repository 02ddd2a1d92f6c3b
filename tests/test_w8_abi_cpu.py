"""The MXFP8 weight-only entry points (CPU): declared by the header, exported by the library, refusing what they cannot run before
any launch; and the build's resource remarks of every gemv_stream_kernel instantiation -- the bf16 ones and the MXFP8 ones share
__launch_bounds__(512, 4): at most 128 VGPRs, and no scratch."""
import ctypes
import os
import re

import pytest

from multimeditron_amd import _lib

BUILD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multimeditron_amd", "csrc", "build")
NEW = ("mm_mxfp8_bytes", "mm_quant_mxfp8", "mm_dequant_mxfp8", "mm_decode_linear_w8", "mm_decode_gateup_swiglu_w8",
       "mm_decode_qkv_rope_append_w8")
UNSUPPORTED, ARG, ALIGN = -3, -1, -2


def test_symbols_declared_and_exported():
    protos = _lib.parse_header()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in protos, f"include/mm_hip.h does not declare {name}"
        assert hasattr(L, name), f"libmmhip.so does not export {name}"
    assert protos["mm_mxfp8_bytes"][0] is ctypes.c_int64
    # the _w8 entry points are the bf16 ones with `packed` in place of (W, ldw)
    for base in ("mm_decode_linear", "mm_decode_gateup_swiglu", "mm_decode_qkv_rope_append"):
        assert len(protos[base + "_w8"][1]) == len(protos[base][1]) - 1


def test_buffer_size():
    L = _lib.lib()
    assert L.mm_mxfp8_bytes(16, 48) == UNSUPPORTED            # K % 32
    assert L.mm_mxfp8_bytes(0, 32) == ARG
    for N, K in ((1, 32), (17, 256), (1003, 4128), (128256, 4096)):
        n = L.mm_mxfp8_bytes(N, K)
        assert n % 16 == 0
        assert n >= N * K + N * (K // 32)                     # the elements and one scale byte per block, at least
        assert n <= 33 * N * (K // 32 + 31) + 16              # ... and the layout's padding: fewer than 32 blocks per row


def test_refusals_come_before_any_launch():
    """K = 48 is no multiple of the block: MM_ERR_UNSUPPORTED from every entry point, on a machine without a GPU too (nothing is
    launched, no device is asked for).  The pointers are never dereferenced."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    assert L.mm_quant_mxfp8(p, 48, 16, 48, p, None) == UNSUPPORTED
    assert L.mm_dequant_mxfp8(p, 16, 48, p, 48, None) == UNSUPPORTED
    assert L.mm_decode_linear_w8(0, 4, 16, 48, p, 48, p, None, None, 0, p, 16, None, 0.0, None) == UNSUPPORTED
    assert L.mm_decode_gateup_swiglu_w8(0, 4, 8, 48, p, 48, p, p, 8, None, 0.0, None) == UNSUPPORTED
    assert L.mm_decode_qkv_rope_append_w8(0, 4, 1, 1, 128, 48, p, 48, p, None, p, 384, p, p, p, p, 384, None, 0.0, None) == UNSUPPORTED
    # x that does not fit the LDS stage (16 rows of 8192 bf16 = 256 KiB)
    assert L.mm_decode_linear_w8(0, 16, 16, 8192, p, 8192, p, None, None, 0, p, 16, None, 0.0, None) == UNSUPPORTED
    # the argument checks of the bf16 entry points hold for the packed ones
    assert L.mm_decode_linear_w8(1, 4, 16, 64, p, 64, p, None, None, 0, p, 16, None, 0.0, None) == UNSUPPORTED     # fp32
    assert L.mm_decode_linear_w8(0, 17, 16, 64, p, 64, p, None, None, 0, p, 16, None, 0.0, None) == ARG            # M > 16
    assert L.mm_decode_linear_w8(0, 4, 16, 64, p, 64, p + 8, None, None, 0, p, 16, None, 0.0, None) == ALIGN
    assert L.mm_quant_mxfp8(p, 60, 16, 64, p, None) == ALIGN                                                        # ldw < K
    assert L.mm_quant_mxfp8(None, 64, 16, 64, p, None) == ARG


def _remarks(path):
    out, cur = {}, None
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, ln)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def test_streaming_kernels_fit_their_launch_bounds():
    path = os.path.join(BUILD, "mm_gemm.o.resources.txt")
    if not os.path.exists(path):
        pytest.skip("library not built in this tree (python multimeditron_amd/csrc/build.py)")
    ks = {n: r for n, r in _remarks(path).items() if "gemv_stream_kernel" in n}
    # 3 modes x NORM x NT, in both weight formats (the last template argument: Lb0E bf16, Lb1E MXFP8)
    assert len(ks) == 24, sorted(ks)
    assert sum(1 for n in ks if n.endswith("Lb1EEEvNS_10SkinnyArgsEi")) == 12, sorted(ks)
    for name, r in sorted(ks.items()):
        assert r["scratch"] == 0, f"{name}: {r['scratch']} bytes/lane of scratch"
        assert r["vgprs"] <= 128, f"{name}: {r['vgprs']} VGPRs"
