// MXFP8 KV cache: the append quantiser and its inverse (include/mm_hip.h: mm_kv8_bytes, mm_kv8_append, mm_kv8_dequant; the format and
// the buffer layout: mm_kv8.h).  As in mm_quant.hip a thread owns 8 consecutive d of one head row (one 16-byte bf16 load, one 8-byte
// store); the 4 threads of a block of 32 find its amax with two xor-shuffles and convert what they loaded.  One pass over the rows,
// K and V in the same launch, nothing but the slots of positions pos .. pos + S - 1 is written.
#include "mm_kv8.h"

namespace {

struct Kv8Rows {          // the bf16 side of both kernels: k / v [B, S, Hkv, 128] through strides in elements (head stride 128)
  bf16 *k, *v;
  int64_t k_sb, k_ss, v_sb, v_ss;
};

// idx -> (K or V, b, s, h, c): c fastest, so the 4 lanes of a block of 32 are neighbours and a wave holds 4 whole head rows
struct Kv8Idx { int isv, b, s, h, c; };
__device__ __forceinline__ Kv8Idx kv8_idx(int64_t idx, int B, int S, int Hkv) {
  Kv8Idx r;
  r.c = (int)(idx & 15);
  int64_t t = idx >> 4;
  r.h = (int)(t % Hkv); t /= Hkv;
  r.s = (int)(t % S); t /= S;
  r.b = (int)(t % B);
  r.isv = (int)(t / B);
  return r;
}

__global__ __launch_bounds__(256) void kv8_append_kernel(Kv8Rows src, int B, int S, int Hkv, unsigned char* cache, Kv8Layout L, int pos) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;            // 2 * B * S * Hkv * 16 threads: a block's 4 lanes are all in or all out
  if (idx >= (int64_t)2 * B * S * Hkv * 16) return;
  const Kv8Idx t = kv8_idx(idx, B, S, Hkv);
  const bf16* row = t.isv ? src.v + t.b * src.v_sb + t.s * src.v_ss : src.k + t.b * src.k_sb + t.s * src.k_ss;
  const u32x4 raw = *(const u32x4*)(row + t.h * 128 + t.c * 8);
  unsigned a16 = mx8_amax16(raw);
  a16 = max(a16, (unsigned)__shfl_xor((int)a16, 1, 64));
  a16 = max(a16, (unsigned)__shfl_xor((int)a16, 2, 64));
  const unsigned byte = mx8_scale_byte(a16);
  const u32x2 q = mx8_from_bf16x8(raw, byte);
  const int64_t bh = (int64_t)t.b * Hkv + t.h, key = pos + t.s;
  *(u32x2*)(cache + (t.isv ? kv8_v_elem(L, bh, key, t.c) : kv8_k_elem(L, bh, key, t.c))) = q;
  if ((t.c & 3) == 0) cache[t.isv ? kv8_v_scale(L, bh, key, t.c >> 2) : kv8_k_scale(L, bh, key, t.c >> 2)] = (unsigned char)byte;
}

__global__ __launch_bounds__(256) void kv8_dequant_kernel(const unsigned char* cache, Kv8Layout L, int pos, Kv8Rows dst, int B, int S, int Hkv) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)2 * B * S * Hkv * 16) return;
  const Kv8Idx t = kv8_idx(idx, B, S, Hkv);
  const int64_t bh = (int64_t)t.b * Hkv + t.h, key = pos + t.s;
  const u32x2 q = *(const u32x2*)(cache + (t.isv ? kv8_v_elem(L, bh, key, t.c) : kv8_k_elem(L, bh, key, t.c)));
  const unsigned byte = cache[t.isv ? kv8_v_scale(L, bh, key, t.c >> 2) : kv8_k_scale(L, bh, key, t.c >> 2)];
  bf16* row = t.isv ? dst.v + t.b * dst.v_sb + t.s * dst.v_ss : dst.k + t.b * dst.k_sb + t.s * dst.k_ss;
  *(bf16x8*)(row + t.h * 128 + t.c * 8) = mx8_to_bf16x8(q, mx8_scale(byte));
}

// the checks both directions share; S rows at positions pos .. pos + S - 1 of a buffer of Smax
int kv8_common(int B, int S, int Hkv, int D, int Smax, int pos, const void* k, const void* v, const void* cache, int64_t s0, int64_t s1,
               int64_t s2, int64_t s3) {
  if (B <= 0 || S <= 0 || Hkv <= 0 || D <= 0 || Smax <= 0 || pos < 0 || (int64_t)pos + S > Smax) return MM_ERR_ARG;
  if (D != 128) return MM_ERR_UNSUPPORTED;
  if (!k || !v || !cache) return MM_ERR_ARG;
  if ((s0 | s1 | s2 | s3) & 7) return MM_ERR_ALIGN;
  if (!mm_aligned16(k) || !mm_aligned16(v) || !mm_aligned16(cache)) return MM_ERR_ALIGN;
  if (((int64_t)2 * B * S * Hkv * 16 + 255) / 256 >= 0x7FFFFFFF) return MM_ERR_UNSUPPORTED;
  return MM_OK;
}

}  // namespace

extern "C" int64_t mm_kv8_bytes(int B, int Smax, int Hkv, int D) {
  if (B <= 0 || Smax <= 0 || Hkv <= 0 || D <= 0) return MM_ERR_ARG;
  if (D != 128) return MM_ERR_UNSUPPORTED;
  return kv8_layout(B, Smax, Hkv).bytes;
}

extern "C" int mm_kv8_append(int dtype, const void* k, const void* v, int B, int S, int Hkv, int D, int64_t k_sb, int64_t k_ss, int64_t v_sb,
                             int64_t v_ss, void* cache, int Smax, int pos, void* stream) {
  if (dtype != MM_BF16) return MM_ERR_UNSUPPORTED;
  const int rc = kv8_common(B, S, Hkv, D, Smax, pos, k, v, cache, k_sb, k_ss, v_sb, v_ss);
  if (rc != MM_OK) return rc;
  const Kv8Rows src{(bf16*)k, (bf16*)v, k_sb, k_ss, v_sb, v_ss};
  const unsigned grid = (unsigned)(((int64_t)2 * B * S * Hkv * 16 + 255) / 256);
  hipLaunchKernelGGL(kv8_append_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, B, S, Hkv, (unsigned char*)cache,
                     kv8_layout(B, Smax, Hkv), pos);
  MM_CHECK_LAUNCH();
  return MM_OK;
}

extern "C" int mm_kv8_dequant(const void* cache, int B, int Smax, int Hkv, int D, int pos, int S, void* k_out, void* v_out, int64_t sb,
                              int64_t ss, void* stream) {
  const int rc = kv8_common(B, S, Hkv, D, Smax, pos, k_out, v_out, cache, sb, ss, 0, 0);
  if (rc != MM_OK) return rc;
  const Kv8Rows dst{(bf16*)k_out, (bf16*)v_out, sb, ss, sb, ss};
  const unsigned grid = (unsigned)(((int64_t)2 * B * S * Hkv * 16 + 255) / 256);
  hipLaunchKernelGGL(kv8_dequant_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)cache, kv8_layout(B, Smax, Hkv),
                     pos, dst, B, S, Hkv);
  MM_CHECK_LAUNCH();
  return MM_OK;
}
