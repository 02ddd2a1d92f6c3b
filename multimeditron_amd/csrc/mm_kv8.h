// MXFP8 KV cache (include/mm_hip.h: mm_kv8_bytes, mm_kv8_append, mm_kv8_dequant, mm_attn_decode_kv8): the format of mm_mxfp8.h -- OCP
// e4m3fn elements, one power-of-two E8M0 scale byte per 32 consecutive d of a head -- applied to the K and V rows [Hkv, D = 128] of
// every cached position.  Shared by the append quantiser and its inverse (mm_kv8.hip) and the decode slice kernel (mm_attn.hip).
//
// The layout of one layer's buffer is private to the library and fixed by (B, Smax, Hkv).  It follows THE LOADS OF
// attn_decode_partial128_mfma_kernel, whose lane (row = l & 15, kq = l >> 4) of a wave that holds 16 keys k0 .. k0 + 15 needs
//   of K: key k0 + row, d = ks * 32 + kq * 8 + j for the four MFMA K-steps ks (j = 0..7) -- 32 bytes, one piece per 32-block;
//   of V: keys k0 + 4 kq + u (u = 0..3), d = row * 8 + j -- 8 bytes of each of four CONSECUTIVE keys, all in block row >> 2.
// With S4 = round_up(Smax, MM_KV8_ALIGN) key slots per (batch, kv head) and bh = b * Hkv + h, the four regions are, in this order:
//   K elements  [B*Hkv][S4][128]         d is PERMUTED inside a key row: byte kq * 32 + ks * 8 + j holds d = ks * 32 + kq * 8 + j, so a
//                                        lane's 32 bytes are contiguous: two 16-byte loads feed the four K-steps with the operands the
//                                        bf16 kernel sees (16 keys of a wave: 2 KiB contiguous)
//   V elements  [B*Hkv][S4/4][16][4][8]  the 8-byte pieces (chunk c = d / 8) of FOUR consecutive keys interleaved: byte
//                                        (key / 4) * 512 + c * 32 + (key & 3) * 8 + j, again 32 contiguous bytes per lane
//   K scales    [B*Hkv][S4][4]           one dword per key: the scales of its blocks 0..3 = of the lane's K-steps 0..3
//   V scales    [B*Hkv][S4/4][4][4]      [block][key & 3]: one dword holds a block's scales of four consecutive keys
// S4 * 264 bytes per (batch, kv head): exactly 1 + 1/32 byte per element, and every region starts 16-byte aligned.
//
// MM_KV8_ALIGN (the A of mm_attn_decode_kv8_chunk): a slice of the keys must start at a multiple of 4, the V interleave.  A lane's V
// load always brings the three partners of a key along, so the partner of the LAST valid key of a slice may be a slot nobody has written
// (NaN bytes, an Inf scale): kv8_v_pieces replaces such a piece and its scale IN REGISTERS by the clamped key's, which is what the bf16
// kernel's address clamp loads -- it is never merely multiplied by a zero probability.
#pragma once
#include "mm_mxfp8.h"

#define MM_KV8_ALIGN 4

struct Kv8Layout {
  int64_t S4;          // key slots per (batch, kv head)
  int64_t ve, ks, vs;  // byte offsets of the V elements, the K scales, the V scales (the K elements start at 0)
  int64_t bytes;       // whole buffer, a multiple of 16
};

__host__ __device__ inline Kv8Layout kv8_layout(int B, int Smax, int Hkv) {
  Kv8Layout L;
  L.S4 = ((int64_t)Smax + MM_KV8_ALIGN - 1) & ~(int64_t)(MM_KV8_ALIGN - 1);
  const int64_t n = (int64_t)B * Hkv * L.S4;
  L.ve = n * 128;
  L.ks = n * 256;
  L.vs = n * 260;
  L.bytes = n * 264;
  return L;
}
// byte offsets inside the regions; bh = b * Hkv + h, c = d / 8 (the 8 elements d = c * 8 .. c * 8 + 7 are contiguous in both regions)
__host__ __device__ inline int64_t kv8_k_elem(const Kv8Layout& L, int64_t bh, int64_t key, int c) {
  return (bh * L.S4 + key) * 128 + (c & 3) * 32 + (c >> 2) * 8;
}
__host__ __device__ inline int64_t kv8_v_elem(const Kv8Layout& L, int64_t bh, int64_t key, int c) {
  return L.ve + (bh * L.S4 + (key & ~(int64_t)3)) * 128 + c * 32 + (key & 3) * 8;
}
__host__ __device__ inline int64_t kv8_k_scale(const Kv8Layout& L, int64_t bh, int64_t key, int blk) {
  return L.ks + (bh * L.S4 + key) * 4 + blk;
}
__host__ __device__ inline int64_t kv8_v_scale(const Kv8Layout& L, int64_t bh, int64_t key, int blk) {
  return L.vs + (bh * L.S4 + (key & ~(int64_t)3)) * 4 + blk * 4 + (key & 3);
}

#ifdef __HIPCC__
// What one lane of the slice kernel holds of a 16-key block, as loaded: 18 registers against the bf16 kernel's 32.
struct Kv8Frag {
  u32x4 k[2];      // K-steps (0, 1) and (2, 3) of the lane's key, 8 bytes each
  u32x4 v[2];      // keys (0, 1) and (2, 3) of the lane's group of four, 8 bytes each
  unsigned ks;     // scale bytes of the K-steps 0..3
  unsigned vs;     // scale bytes of the keys 0..3
};

__device__ __forceinline__ bf16x8 kv8_k_piece(const Kv8Frag& f, int ks) {
  const u32x2 q = {f.k[ks >> 1][(ks & 1) * 2], f.k[ks >> 1][(ks & 1) * 2 + 1]};
  return mx8_to_bf16x8(q, mx8_scale((f.ks >> (8 * ks)) & 255u));
}
// The four V fragments of a lane whose keys are g0 .. g0 + 3 (g0 a multiple of 4) in a slice whose last key is `last`: fragment u is
// key min(g0 + u, last), the bf16 kernel's address clamp.  The load brought the group of min(g0, last & ~3); a key past `last` takes
// the bytes and the scale of key `last` before anything is converted.
__device__ __forceinline__ void kv8_v_pieces(const Kv8Frag& f, int g0, int last, bf16x8 (&vf)[4]) {
  u32x2 q[4];
  unsigned sb[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    q[u] = u32x2{f.v[u >> 1][(u & 1) * 2], f.v[u >> 1][(u & 1) * 2 + 1]};
    sb[u] = (f.vs >> (8 * u)) & 255u;
  }
  const int hi = last - min(g0, last & ~3);          // index of the last key inside the loaded group, >= 0 (above 3: no key is clamped)
  const int lo = g0 > last ? hi : 0;                 // a group wholly past the slice: every fragment is key `last`
#pragma unroll
  for (int u = 2; u >= 0; --u)
    if (u < lo) { q[u] = q[u + 1]; sb[u] = sb[u + 1]; }
#pragma unroll
  for (int u = 1; u < 4; ++u)
    if (u > hi) { q[u] = q[u - 1]; sb[u] = sb[u - 1]; }
#pragma unroll
  for (int u = 0; u < 4; ++u) vf[u] = mx8_to_bf16x8(q[u], mx8_scale(sb[u]));
}
#endif
