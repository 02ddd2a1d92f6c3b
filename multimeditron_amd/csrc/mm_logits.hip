// Logits processors of generate() on the device: repetition penalty -> n-gram ban -> minimum length -> suppressed ids, transformers'
// order (RepetitionPenalty / NoRepeatNGram / MinNewTokensLength / SuppressTokens LogitsProcessor), from bf16 or fp32 logits to fp32
// scores in ONE launch per step.  The contract is written out in include/mm_hip.h (mm_logits_process); tests/logits_ref.py restates
// it in numpy.
//
// Grid: rows x ceil(V / 4096) workgroups (the vocabulary cut into chunks, as mm_sample / mm_beam_step cut theirs), 256 threads.  A
// workgroup
//   1. zeroes two 4096-bit maps of its chunk in LDS: "seen" (ids of the row's history) and "banned" (-inf);
//   2. scans the row's whole history (plen + step int32 ids, L2-resident: every chunk of the row reads the same ints) and sets the
//      bits of the ids that fall into its chunk with integer LDS atomics (order-free: the same maps on every launch); an n-gram start
//      is compared with the tail only when the id it would ban lies in the chunk;
//   3. makes one pass over its chunk: load, penalise from "seen", -inf from "banned", store fp32.  Thread t takes entries
//      k * 1024 + 4 t .. + 3 (k = 0 .. 3): a 16-byte store (8- or 16-byte load) per lane, consecutive lanes on consecutive addresses.
// The penalty is computed from the loaded value, so a repeated id is penalised once; nothing is read back through global memory.  The
// newest id comes from last_ids in every workgroup; chunk 0 of a row stores it into hist for the later steps (no workgroup of this
// launch reads that slot).
#include "mm_common.h"

namespace {

constexpr int LCHUNK = 4096;               // vocabulary entries per workgroup
constexpr int LWORDS = LCHUNK / 32;        // words of a bit map
constexpr int LGROUP = 4;                  // contiguous entries per thread and round
constexpr int LROUNDS = LCHUNK / (256 * LGROUP);

struct LArgs {
  const void* logits;
  int V, ld, C, vec;
  int step, ld_hist, max_plen;
  const int64_t* last_ids;
  int32_t* hist;
  const int32_t* plen;
  float p;
  int pen, g;                // pen: repetition penalty on (p != 1)
  int ban_eos;               // eos while step < min_new_tokens, else -1
  const int32_t* suppress;
  int n_suppress;
  float* out;
  int ld_out;
};

template <typename T> struct Vec4;
template <> struct Vec4<bf16> { typedef bf16x4 type; };
template <> struct Vec4<float> { typedef f32x4 type; };

__device__ __forceinline__ void set_bit(unsigned* map, int id, int v0, int v1) {
  if (id >= v0 && id < v1) atomicOr(&map[(id - v0) >> 5], 1u << ((id - v0) & 31));
}

template <typename T>
__global__ __launch_bounds__(256) void logits_process_kernel(LArgs a) {
  __shared__ unsigned seen[LWORDS];
  __shared__ unsigned banned[LWORDS];
  const int r = (int)(blockIdx.x / (unsigned)a.C), c = (int)(blockIdx.x % (unsigned)a.C);
  const int tid = threadIdx.x;
  const int v0 = c * LCHUNK, v1 = min(v0 + LCHUNK, a.V);      // ids outside [v0, v1) set no bit: nothing outside [0, V) indexes a row
  if (tid < LWORDS) { seen[tid] = 0u; banned[tid] = 0u; }
  __syncthreads();

  if (a.hist) {
    const int pl = min(max(a.plen[r], 0), a.max_plen);         // keeps every index below inside the row of hist
    const int L = pl + a.step;
    int32_t* h = a.hist + (int64_t)r * a.ld_hist;
    const int32_t last = a.step > 0 ? (int32_t)a.last_ids[r] : 0;
    // entry j of the history; the newest one (step > 0) is not in hist yet
    auto hget = [&](int j) -> int32_t { return (a.step > 0 && j == L - 1) ? last : h[j]; };
    if (a.step > 0 && c == 0 && tid == 0) h[L - 1] = last;
    if (a.pen)
      for (int j = tid; j < L; j += 256) set_bit(seen, hget(j), v0, v1);
    const int g = a.g;
    if (g > 0 && L + 1 >= g) {
      const int t0 = L - g + 1;                                // the tail h[t0 .. L-1] (g - 1 ids)
      for (int i = tid; i <= L - g; i += 256) {
        const int32_t cand = hget(i + g - 1);
        if (cand < v0 || cand >= v1) continue;
        bool same = true;
        for (int k = 0; k < g - 1 && same; ++k) same = hget(i + k) == hget(t0 + k);
        if (same) set_bit(banned, cand, v0, v1);
      }
    }
  }
  if (tid == 0 && a.ban_eos >= 0) set_bit(banned, a.ban_eos, v0, v1);
  for (int j = tid; j < a.n_suppress; j += 256) set_bit(banned, a.suppress[j], v0, v1);
  __syncthreads();

  const T* row = (const T*)a.logits + (int64_t)r * a.ld;
  float* orow = a.out + (int64_t)r * a.ld_out;
  const float p = a.p;
#pragma unroll
  for (int k = 0; k < LROUNDS; ++k) {
    const int q = k * 256 * LGROUP + tid * LGROUP;             // first entry of the group inside the chunk
    const int e0 = v0 + q;
    const int n = min(LGROUP, a.V - e0);
    if (n <= 0) continue;
    const unsigned sb = (seen[q >> 5] >> (q & 31)) & 0xFu, bb = (banned[q >> 5] >> (q & 31)) & 0xFu;
    float x[LGROUP];
    const bool wide = a.vec && n == LGROUP;
    if (wide) {
      const typename Vec4<T>::type v = *(const typename Vec4<T>::type*)(row + e0);
#pragma unroll
      for (int j = 0; j < LGROUP; ++j) x[j] = (float)v[j];
    } else {
#pragma unroll
      for (int j = 0; j < LGROUP; ++j) x[j] = j < n ? to_f32(row[e0 + j]) : 0.f;
    }
#pragma unroll
    for (int j = 0; j < LGROUP; ++j) {
      if ((sb >> j) & 1u) x[j] = x[j] < 0.f ? __fmul_rn(x[j], p) : __fdiv_rn(x[j], p);
      if ((bb >> j) & 1u) x[j] = -INFINITY;
    }
    if (wide) {
      f32x4 o = {x[0], x[1], x[2], x[3]};
      *(f32x4*)(orow + e0) = o;
    } else {
#pragma unroll
      for (int j = 0; j < LGROUP; ++j)
        if (j < n) orow[e0 + j] = x[j];
    }
  }
}

}  // namespace

extern "C" int mm_logits_process(int dtype, const void* logits, int rows, int V, int ld, int step, const int64_t* last_ids,
                                 int32_t* hist, int ld_hist, const int32_t* plen, int max_plen, float repetition_penalty,
                                 int no_repeat_ngram_size, int min_new_tokens, int64_t eos, const int32_t* suppress, int n_suppress,
                                 float* out, int ld_out, void* stream) {
  if (dtype != MM_BF16 && dtype != MM_F32) return MM_ERR_ARG;
  const float p = repetition_penalty;
  if (!(p > 0.f) || !(p < INFINITY)) return MM_ERR_ARG;      // NaN fails both
  if (no_repeat_ngram_size < 0 || min_new_tokens < 0 || step < 0 || rows < 0 || n_suppress < 0) return MM_ERR_ARG;
  if (V <= 0 || ld < V || ld_out < V) return MM_ERR_ARG;
  if (step < min_new_tokens && (eos < 0 || eos >= V)) return MM_ERR_ARG;
  if (!logits || !out || (const void*)out == logits) return MM_ERR_ARG;
  if (n_suppress > 0 && !suppress) return MM_ERR_ARG;
  const bool need_hist = p != 1.f || no_repeat_ngram_size > 0;
  if (need_hist && (!hist || !plen)) return MM_ERR_ARG;
  if (hist) {
    if (!plen || max_plen < 0 || ld_hist < 0 || (int64_t)max_plen + step > ld_hist) return MM_ERR_ARG;
    if (step > 0 && !last_ids) return MM_ERR_ARG;
  }
  const int64_t C = ((int64_t)V + LCHUNK - 1) / LCHUNK;
  if (C * rows > 0x7FFFFFFFll) return MM_ERR_ARG;
  if (rows == 0) return MM_OK;
  LArgs a;
  a.logits = logits;
  a.V = V;
  a.ld = ld;
  a.C = (int)C;
  a.vec = mm_aligned16(logits) && ((int64_t)ld * mm_elem_size(dtype)) % 16 == 0 && mm_aligned16(out) && ld_out % 4 == 0;
  a.step = step;
  a.ld_hist = ld_hist;
  a.max_plen = max_plen;
  a.last_ids = last_ids;
  a.hist = hist;
  a.plen = plen;
  a.p = p;
  a.pen = p != 1.f;
  a.g = no_repeat_ngram_size;
  a.ban_eos = step < min_new_tokens ? (int)eos : -1;
  a.suppress = suppress;
  a.n_suppress = n_suppress;
  a.out = out;
  a.ld_out = ld_out;
  const dim3 grid((unsigned)(C * rows)), block(256);
  if (dtype == MM_BF16)
    hipLaunchKernelGGL(logits_process_kernel<bf16>, grid, block, 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(logits_process_kernel<float>, grid, block, 0, (hipStream_t)stream, a);
  MM_CHECK_LAUNCH();
  return MM_OK;
}
