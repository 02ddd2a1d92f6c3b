"""mm_gemm_mx8 / mm_gemm_mx8_supported (CPU): declared by the header, exported by the library, answering the documented codes
without a GPU; the build's resource remarks of the kernel (no scratch, no more registers than __launch_bounds__(512) leaves a
wave: 256); and the packed layout of the K widths the prefill needs, which must carry no padding slots."""
import ctypes
import os
import re

import pytest

from multimeditron_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "multimeditron_amd", "csrc", "build")
OK, ARG, ALIGN, UNSUPPORTED = 0, -1, -2, -3
BIAS, GELU, RES, ACC = 1, 2, 8, 16
REQUIRED_K = (2048, 4096, 8192, 14336, 21504)      # Llama-3.2-1B, Llama-3.1-8B, Apertus-8B


def test_symbols_declared_and_exported():
    protos = _lib.parse_header()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mm_gemm_mx8", "mm_gemm_mx8_supported"):
        assert name in protos, f"include/mm_hip.h does not declare {name}"
        assert hasattr(L, name), f"libmmhip.so does not export {name}"
    assert len(protos["mm_gemm_mx8"][1]) == 12 and len(protos["mm_gemm_mx8_supported"][1]) == 3
    hdr = open(_lib.HEADER).read()
    assert "23 the MXFP8 x MXFP8" in hdr                       # the id "gemm_last_kernel" reports is documented


def test_supported_answers_without_a_device():
    L = _lib.lib()
    for K in REQUIRED_K + (128, 384, 3584, 18944, 2560, 9728):
        for M, N in ((1, 1), (74, 6144), (8192, 28672)):
            assert L.mm_gemm_mx8_supported(M, N, K) == OK, (M, N, K)
    assert L.mm_gemm_mx8_supported(16, 16, 96) == UNSUPPORTED
    assert L.mm_gemm_mx8_supported(16, 16, 64) == UNSUPPORTED
    assert L.mm_gemm_mx8_supported(16, 16, (1 << 20) + 128) == UNSUPPORTED
    assert L.mm_gemm_mx8_supported(0, 16, 128) == ARG
    assert L.mm_gemm_mx8_supported(16, -1, 128) == ARG
    assert L.mm_gemm_mx8_supported(16, 16, 0) == ARG


def test_refusals_come_before_any_launch():
    """No pointer is dereferenced and no device is asked for."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    assert L.mm_gemm_mx8(16, 16, 96, p, p, None, None, 0, p, 16, 0, None) == UNSUPPORTED
    for epi in (GELU, ACC, BIAS | GELU, 64):
        assert L.mm_gemm_mx8(16, 16, 128, p, p, p, p, 16, p, 16, epi, None) == UNSUPPORTED
    assert L.mm_gemm_mx8(16, 16, 128, None, p, None, None, 0, p, 16, 0, None) == ARG
    assert L.mm_gemm_mx8(16, 16, 128, p, p, None, None, 0, p, 8, 0, None) == ARG             # ldc < N
    assert L.mm_gemm_mx8(16, 16, 128, p, p, None, None, 0, p, 16, BIAS, None) == ARG         # the bit without the vector
    assert L.mm_gemm_mx8(16, 16, 128, p, p, None, p, 8, p, 16, RES, None) == ARG             # ldr < N
    assert L.mm_gemm_mx8(16, 16, 128, p + 8, p, None, None, 0, p, 16, 0, None) == ALIGN
    assert L.mm_gemm_mx8(16, 16, 128, p, p + 4, None, None, 0, p, 16, 0, None) == ALIGN


def _layout():
    """per / sper of csrc/mm_mxfp8.h's mx8_layout, read from the header's own expressions"""
    src = open(os.path.join(ROOT, "multimeditron_amd", "csrc", "mm_mxfp8.h")).read()
    assert "L.per = (nks + 7) / 8;" in src and "L.sper = (L.per + 3) & ~3;" in src and "const int nks = K / 32;" in src
    return lambda K: ((K // 32 + 7) // 8, ((K // 32 + 7) // 8 + 3) & ~3)


def test_required_widths_have_no_padding_slots():
    layout = _layout()
    L = _lib.lib()
    for K in REQUIRED_K:
        per, sper = layout(K)
        assert per % 4 == 0 and sper == per and 8 * per * 32 == K, (K, per, sper)
        for N in (1, 74, 4096):
            assert L.mm_mxfp8_bytes(N, K) == (N * K + N * (K // 32) + 15) // 16 * 16        # 1 + 1/32 byte per element, nothing else
    for K in (3584, 18944, 2560, 9728, 128, 384):                                          # ... and these do (taken all the same)
        per, sper = layout(K)
        assert 8 * sper * 32 > K
        assert L.mm_mxfp8_bytes(16, K) > 16 * K + 16 * (K // 32) + 15


def _remarks(path):
    out, cur = {}, None
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("agprs", r" AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, ln)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def test_kernel_fits_its_launch_bounds_without_scratch():
    path = os.path.join(BUILD, "mm_gemm_mx8.o.resources.txt")
    if not os.path.exists(path):
        pytest.skip("library not built in this tree (python multimeditron_amd/csrc/build.py)")
    ks = {n: r for n, r in _remarks(path).items() if "gemm_mx8_kernel" in n}
    assert len(ks) == 1, sorted(ks)
    for name, r in ks.items():
        assert r["scratch"] == 0, f"{name}: {r['scratch']} bytes/lane of scratch"
        assert r["vgprs"] <= 256 and r["vgprs"] + r["agprs"] <= 512, f"{name}: {r}"      # 512 threads: 2 waves per SIMD
