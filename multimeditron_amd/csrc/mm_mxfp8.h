// MXFP8 weight-only storage (include/mm_hip.h: mm_quant_mxfp8): OCP e4m3fn elements, one power-of-two E8M0 scale byte per 32
// consecutive k of a row.  Shared by the quantiser (mm_quant.hip) and the decode kernel that streams the bytes (mm_gemm.hip); the
// element / scale conversions at the end also serve the MXFP8 KV cache (mm_kv8.h), which has its own layout.
//
// The layout of the packed buffer is private to the library and fixed by (N, K) alone.  It follows THE ORDER THE KERNEL WALKS W:
// gemv_stream_kernel gives wave w of a workgroup the K-steps (blocks of 32) w*per .. w*per + per - 1, per = ceil(K/32 / 8), and a lane
// the 8 consecutive k (kc = 0..3) of a step as its bf16x8 MFMA fragment.  Row n is 8 runs (one per wave) of sper = round_up(per, 4)
// step slots; slot i of run w is the wave's step i (a slot past the wave's last step is padding: zero elements, scale 2^0).
//   [0, N*8*sper*32)     the elements, 32 bytes per slot, two slots interleaved per 64 bytes so that ONE 16-byte load of a lane
//                        feeds two MFMA steps (8-byte loads -- 32-byte row segments -- ran at the bf16 kernel's time per load, not per
//                        byte): slot pair p is [kc 0: step 2p | step 2p+1][kc 1: ..][kc 2][kc 3], 8 bytes each
//   [.., + N*8*sper)     the scale bytes, slot by slot: the dword with the scales of a wave's steps i .. i+3 is 4-byte aligned
// K-widths whose per is a multiple of 4 (4096, 14336, ...) carry no padding: 1 + 1/32 byte per weight.
#pragma once
#include "mm_common.h"

struct Mx8Layout {
  int per;              // K-steps per wave of gemv_stream_kernel
  int sper;             // step slots per (row, wave) run
  int64_t scale_off;    // byte offset of the scales
  int64_t bytes;        // whole buffer, a multiple of 16
};

__host__ __device__ inline Mx8Layout mx8_layout(int N, int K) {
  Mx8Layout L;
  const int nks = K / 32;
  L.per = (nks + 7) / 8;
  L.sper = (L.per + 3) & ~3;
  L.scale_off = (int64_t)N * 8 * L.sper * 32;
  L.bytes = (L.scale_off + (int64_t)N * 8 * L.sper + 15) & ~(int64_t)15;
  return L;
}
// byte offset of the 8 elements (slot i of run `run` = row * 8 + wave, k-chunk kc) / of the slot's scale byte behind scale_off
__host__ __device__ inline int64_t mx8_elem_off(const Mx8Layout& L, int64_t run, int i, int kc) {
  return (run * L.sper + (i & ~1)) * 32 + kc * 16 + (i & 1) * 8;
}

#ifdef __HIPCC__
// 2^(byte - 127) as fp32; byte in [27, 254] (the quantiser's clamp) is a normal number
__device__ __forceinline__ float mx8_scale(unsigned byte) { return __builtin_bit_cast(float, byte << 23); }

// 8 e4m3 bytes times the block's scale -> the bf16x8 fragment, two elements per v_cvt_scalef32_pk_bf16_fp8 (gfx950's MX conversion:
// fp8 -> bf16 with an fp32 scale).  An e4m3 value has at most 4 significant bits and the product with a power of two stays a normal
// number (or a zero, sign kept), so the result IS the product: no rounding anywhere.
__device__ __forceinline__ bf16x8 mx8_to_bf16x8(u32x2 q, float sc) {
  const u32x4 r = {__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[0], sc, false)),
                   __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[0], sc, true)),
                   __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[1], sc, false)),
                   __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[1], sc, true))};
  return __builtin_bit_cast(bf16x8, r);
}
// Scale byte of a block from the largest |w| as a bf16 bit pattern (sign cleared).  a16 orders like the magnitude, and
// floor(log2 amax) and "amax * 2^-e0 > 448" are read from its fields: amax * 2^-e0 = 1.m * 2^8, above 448 = 1.75 * 2^8 when the 7
// mantissa bits exceed 0x60.  A subnormal amax (exponent field 0) lands below the lower clamp like every amax < 2^-92.
__device__ __forceinline__ unsigned mx8_scale_byte(unsigned a16) {
  if (a16 == 0) return 127u;
  const int e = (int)(a16 >> 7) - 127 - 8 + ((a16 & 0x7Fu) > 0x60u ? 1 : 0);
  return (unsigned)min(max(e + 127, 27), 254);
}
// largest |w| of 8 bf16 (one 16-byte load) as that bit pattern
__device__ __forceinline__ unsigned mx8_amax16(u32x4 raw) {
  unsigned a16 = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) a16 = max(a16, max(raw[e] & 0x7FFFu, (raw[e] >> 16) & 0x7FFFu));
  return a16;
}
// 8 bf16 under their block's scale byte -> 8 e4m3 bytes: round to nearest even, sign of zero kept
__device__ __forceinline__ u32x2 mx8_from_bf16x8(u32x4 raw, unsigned byte) {
  const float inv = __builtin_bit_cast(float, (254u - byte) << 23);          // 2^-e, exact
  const bf16x8 wv = __builtin_bit_cast(bf16x8, raw);
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = fmaxf(-448.f, fminf((float)wv[e] * inv, 448.f));      // never active; keeps the sign of zero
  u32x2 q;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * h], v[4 * h + 1], 0, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * h + 2], v[4 * h + 3], p, true);
    q[h] = (unsigned)p;
  }
  return q;
}
#endif
