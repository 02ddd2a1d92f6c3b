// MXFP8 weight-only quantiser and its inverse (include/mm_hip.h: mm_mxfp8_bytes, mm_quant_mxfp8, mm_dequant_mxfp8; the format and the
// buffer layout: mm_mxfp8.h).  A thread owns 8 consecutive k of one row (one 16-byte bf16 load, one 8-byte store); the 4 threads of
// a block of 32 find its amax with two xor-shuffles and convert what they loaded: one pass over W, written in the layout's order.
#include "mm_mxfp8.h"

namespace {

// One thread per (row, wave run, step slot, kc): the slots of the layout, padding included, so every byte of the buffer is written.
__global__ __launch_bounds__(256) void quant_mxfp8_kernel(const bf16* W, int ldw, int N, int K, unsigned char* packed, Mx8Layout L) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;            // a slot's 4 lanes (kc) are all in or all out
  if (idx >= (int64_t)N * 8 * L.sper * 4) return;
  const int kc = (int)(idx & 3);
  const int64_t slot = idx >> 2, run = slot / L.sper;
  const int i = (int)(slot - run * L.sper), row = (int)(run >> 3), ks = (int)(run & 7) * L.per + i;
  const bool real = i < L.per && ks < K / 32;                              // uniform over the 4 lanes
  u32x4 raw = {0u, 0u, 0u, 0u};
  if (real) raw = *(const u32x4*)(W + (int64_t)row * ldw + ks * 32 + kc * 8);
  unsigned a16 = mx8_amax16(raw);
  a16 = max(a16, (unsigned)__shfl_xor((int)a16, 1, 64));
  a16 = max(a16, (unsigned)__shfl_xor((int)a16, 2, 64));
  const unsigned byte = mx8_scale_byte(a16);                                // a padding slot: zeros, byte 127
  const u32x2 q = mx8_from_bf16x8(raw, byte);
  *(u32x2*)(packed + mx8_elem_off(L, run, i, kc)) = q;
  if (kc == 0) packed[L.scale_off + slot] = (unsigned char)byte;
  if (idx == 0)                                                              // the tail up to the 16-byte multiple
    for (int64_t p = L.scale_off + (int64_t)N * 8 * L.sper; p < L.bytes; ++p) packed[p] = 0;
}

__global__ __launch_bounds__(256) void dequant_mxfp8_kernel(const unsigned char* packed, int N, int K, bf16* Wd, int ldd, Mx8Layout L) {
  const int cpr = K / 8;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)N * cpr) return;
  const int row = (int)(idx / cpr), c = (int)(idx - (int64_t)row * cpr);
  const int ks = c >> 2, wv8 = ks / L.per, i = ks - wv8 * L.per;
  const int64_t run = (int64_t)row * 8 + wv8;
  const unsigned byte = packed[L.scale_off + run * L.sper + i];
  const u32x2 q = *(const u32x2*)(packed + mx8_elem_off(L, run, i, c & 3));
  *(bf16x8*)(Wd + (int64_t)row * ldd + c * 8) = mx8_to_bf16x8(q, mx8_scale(byte));
}

}  // namespace

extern "C" int64_t mm_mxfp8_bytes(int N, int K) {
  if (N <= 0 || K <= 0) return MM_ERR_ARG;
  if (K % 32) return MM_ERR_UNSUPPORTED;
  return mx8_layout(N, K).bytes;
}

static int mx8_common(const void* W, int ld, int N, int K, const void* packed) {
  if (N <= 0 || K <= 0 || !W || !packed) return MM_ERR_ARG;
  if (K % 32) return MM_ERR_UNSUPPORTED;
  if (ld < K || (ld & 7) || !mm_aligned16(W) || !mm_aligned16(packed)) return MM_ERR_ALIGN;
  if ((int64_t)N * (K / 8) + 255 >= (int64_t)0x7FFFFFFF * 256) return MM_ERR_UNSUPPORTED;
  return MM_OK;
}

extern "C" int mm_quant_mxfp8(const void* W, int ldw, int N, int K, void* packed, void* stream) {
  const int rc = mx8_common(W, ldw, N, K, packed);
  if (rc != MM_OK) return rc;
  const Mx8Layout L = mx8_layout(N, K);
  const int64_t nblk = ((int64_t)N * 8 * L.sper * 4 + 255) / 256;
  if (nblk >= 0x7FFFFFFF) return MM_ERR_UNSUPPORTED;
  const unsigned grid = (unsigned)nblk;
  hipLaunchKernelGGL(quant_mxfp8_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16*)W, ldw, N, K, (unsigned char*)packed,
                     mx8_layout(N, K));
  MM_CHECK_LAUNCH();
  return MM_OK;
}

extern "C" int mm_dequant_mxfp8(const void* packed, int N, int K, void* Wd, int ldd, void* stream) {
  const int rc = mx8_common(Wd, ldd, N, K, packed);
  if (rc != MM_OK) return rc;
  const unsigned grid = (unsigned)(((int64_t)N * (K / 8) + 255) / 256);
  hipLaunchKernelGGL(dequant_mxfp8_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)packed, N, K, (bf16*)Wd, ldd,
                     mx8_layout(N, K));
  MM_CHECK_LAUNCH();
  return MM_OK;
}
