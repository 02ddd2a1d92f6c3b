// Classifier-free guidance of generate(guidance_scale=): transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor on the device,
// from the conditional and the unconditional logits rows of ONE decoder pass (bf16 or fp32) to fp32 scores.  The contract is written
// out in include/mm_hip.h (mm_cfg_combine); tests/cfg_check.py restates it in fp64.
//
// Two short launches, handed over at the launch boundary (no atomics, no arrival counters: fixed reduction orders, the same bits on
// every launch):
//   cfg_part_kernel      ceil(V / 4096) x 2 rows workgroups (the conditional rows first), one thread per 16 contiguous logits
//                        (beam_part_kernel's cut): the chunk's maximum and its sum of exp(x - max)
//   cfg_combine_kernel   ceil(V / 4096) x rows workgroups: threads 0 and 1 rebuild the two log-sum-exp of the pair from the partials
//                        in chunk order (every workgroup of a pair computes the same two numbers); every thread then re-reads its 16
//                        entries of both rows (8 / 16 KiB per workgroup and row) and stores 16 fp32 scores
#include "mm_common.h"

#include <math.h>

namespace {

constexpr int GCHUNK = 4096;               // vocabulary entries per workgroup
constexpr int GPT = GCHUNK / 256;          // 16 contiguous entries per thread
constexpr int GMAXV = 1 << 24;

struct GArgs {
  const void* cond;
  const void* uncond;
  int ld_c, ld_u, vec_c, vec_u;
  int rows, V, C;
  float scale;
  float* cmax;               // [2 rows, C]: the conditional rows, then the unconditional ones
  float* csum;               // [2 rows, C]
  float* out;
  int ld_out, vec_o;
};

// the thread's 16 entries of a row; entries from nv on (columns >= V) are not read
template <typename T>
__device__ __forceinline__ void load16(const T* row, int e0, int nv, bool vec, float* x) {
  if (vec && nv == GPT) {
    constexpr int N = Vec16<T>::N;
    const Vec16<T>* p = (const Vec16<T>*)(row + e0);
#pragma unroll
    for (int i = 0; i < GPT / N; ++i) {
      const Vec16<T> v = p[i];
#pragma unroll
      for (int j = 0; j < N; ++j) x[i * N + j] = v.get(j);
    }
  } else {
#pragma unroll
    for (int j = 0; j < GPT; ++j) x[j] = j < nv ? to_f32(row[e0 + j]) : -INFINITY;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void cfg_part_kernel(GArgs a) {
  __shared__ float red[4];
  const int c = blockIdx.x, r = blockIdx.y;                // r in [0, 2 rows)
  const bool un = r >= a.rows;
  const T* row = un ? (const T*)a.uncond + (int64_t)(r - a.rows) * a.ld_u : (const T*)a.cond + (int64_t)r * a.ld_c;
  const int e0 = c * GCHUNK + (int)threadIdx.x * GPT;
  const int nv = min(GPT, a.V - e0);                       // <= 0: this thread has no entry
  float x[GPT];
  load16<T>(row, e0, nv, un ? a.vec_u : a.vec_c, x);
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < GPT; ++j)
    if (j < nv) mx = fmaxf(mx, x[j]);
  mx = block_max_256(mx, red);
  float sm = 0.f;
#pragma unroll
  for (int j = 0; j < GPT; ++j)
    if (j < nv && x[j] > -INFINITY) sm += expf(x[j] - mx);
  sm = block_sum_256(sm, red);
  if (threadIdx.x == 0) {
    a.cmax[(int64_t)r * a.C + c] = mx;
    a.csum[(int64_t)r * a.C + c] = sm;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void cfg_combine_kernel(GArgs a) {
  __shared__ float lse[2];
  const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  if (tid < 2) {
    const int64_t pr = tid == 0 ? r : a.rows + r;
    const float* cm = a.cmax + pr * a.C;
    const float* cs = a.csum + pr * a.C;
    float m = -INFINITY;
    for (int k = 0; k < a.C; ++k) m = fmaxf(m, cm[k]);
    float s = 0.f;
    for (int k = 0; k < a.C; ++k)
      if (cm[k] > -INFINITY) s += cs[k] * expf(cm[k] - m);   // chunk order
    lse[tid] = m + logf(s);
  }
  __syncthreads();
  const int e0 = c * GCHUNK + tid * GPT;
  const int nv = min(GPT, a.V - e0);
  if (nv <= 0) return;
  float xc[GPT], xu[GPT];
  load16<T>((const T*)a.cond + (int64_t)r * a.ld_c, e0, nv, a.vec_c, xc);
  load16<T>((const T*)a.uncond + (int64_t)r * a.ld_u, e0, nv, a.vec_u, xu);
  const float lc = lse[0], lu = lse[1], sc = a.scale;
  float o[GPT];
#pragma unroll
  for (int j = 0; j < GPT; ++j) {
    const float yc = __fsub_rn(xc[j], lc), yu = __fsub_rn(xu[j], lu);
    o[j] = __fadd_rn(__fmul_rn(sc, __fsub_rn(yc, yu)), yu);  // three roundings, never a fused multiply-add: HF's formula
  }
  float* orow = a.out + (int64_t)r * a.ld_out + e0;
  if (a.vec_o && nv == GPT) {
#pragma unroll
    for (int i = 0; i < GPT / 4; ++i) {
      const f32x4 v = {o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]};
      *(f32x4*)(orow + 4 * i) = v;
    }
  } else {
#pragma unroll
    for (int j = 0; j < GPT; ++j)
      if (j < nv) orow[j] = o[j];
  }
}

inline int64_t cfg_chunks(int V) { return ((int64_t)V + GCHUNK - 1) / GCHUNK; }
inline int64_t cfg_bytes(int rows, int V) { return (2 * 2 * (int64_t)rows * cfg_chunks(V) * (int64_t)sizeof(float) + 15) / 16 * 16; }

}  // namespace

extern "C" int mm_cfg_ws_bytes(int rows, int V, int64_t* bytes) {
  if (rows < 0 || V <= 0 || V > GMAXV || !bytes) return MM_ERR_ARG;
  *bytes = cfg_bytes(rows, V);
  return MM_OK;
}

extern "C" int mm_cfg_combine(int dtype, const void* cond, int ld_c, const void* uncond, int ld_u, int rows, int V, float scale,
                              float* out, int ld_out, void* ws, int64_t ws_bytes, void* stream) {
  if (dtype != MM_BF16 && dtype != MM_F32) return MM_ERR_ARG;
  if (rows < 0 || rows > 32767 || V <= 0 || V > GMAXV) return MM_ERR_ARG;     // 2 rows index a grid dimension
  if (ld_c < V || ld_u < V || ld_out < V) return MM_ERR_ARG;
  if (!(fabsf(scale) < INFINITY)) return MM_ERR_ARG;                         // NaN fails it too
  if (!cond || !uncond || !out || !ws) return MM_ERR_ARG;
  if ((const void*)out == cond || (const void*)out == uncond) return MM_ERR_ARG;
  if (ws_bytes < cfg_bytes(rows, V)) return MM_ERR_ARG;
  if (!mm_aligned16(ws)) return MM_ERR_ALIGN;
  if (rows == 0) return MM_OK;
  const int es = mm_elem_size(dtype);
  GArgs a;
  a.cond = cond;
  a.uncond = uncond;
  a.ld_c = ld_c;
  a.ld_u = ld_u;
  a.vec_c = mm_aligned16(cond) && ((int64_t)ld_c * es) % 16 == 0;
  a.vec_u = mm_aligned16(uncond) && ((int64_t)ld_u * es) % 16 == 0;
  a.rows = rows;
  a.V = V;
  a.C = (int)cfg_chunks(V);
  a.scale = scale;
  a.cmax = (float*)ws;
  a.csum = a.cmax + 2 * (int64_t)rows * a.C;
  a.out = out;
  a.ld_out = ld_out;
  a.vec_o = mm_aligned16(out) && ld_out % 4 == 0;
  const dim3 block(256), gpart((unsigned)a.C, (unsigned)(2 * rows)), gcomb((unsigned)a.C, (unsigned)rows);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MM_BF16) {
    hipLaunchKernelGGL(cfg_part_kernel<bf16>, gpart, block, 0, s, a);
    hipLaunchKernelGGL(cfg_combine_kernel<bf16>, gcomb, block, 0, s, a);
  } else {
    hipLaunchKernelGGL(cfg_part_kernel<float>, gpart, block, 0, s, a);
    hipLaunchKernelGGL(cfg_combine_kernel<float>, gcomb, block, 0, s, a);
  }
  MM_CHECK_LAUNCH();
  return MM_OK;
}
