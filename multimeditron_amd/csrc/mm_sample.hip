// Seeded top-k / top-p / min-p sampling of the next token on the device: generate(do_sample=True, top_k=, top_p=, min_p=,
// seed=) (HF warper order temperature -> top-k -> top-p -> min-p, transformers generation/utils.py).  The contract is written
// out in include/mm_hip.h (mm_sample); tests/sampling_ref.py restates it in fp64.
//
// Every launch runs over rows x ceil(V / 4096) workgroups (the vocabulary cut into chunks, like argmax_part/pick in
// mm_rowwise.hip), one thread per 16 contiguous entries:
//   sample_max_kernel     chunk maxima of x = logit / T; zeroes the row's histograms
//   sample_hist_kernel    one radix-select pass (per select: 11 / 11 / 10-bit digits of an order-preserving key of x): every
//                         workgroup first resolves the previous pass from its histogram (redundantly, identically; workgroup 0
//                         stores the result for the next launch), then adds its chunk to this pass's histogram.  top-k selects
//                         on counts, top-p on mass; with both on, top-p runs its three passes over the set top-k kept.
//   sample_mass_kernel    resolves the last pass; kept mass and smallest kept key of each chunk
//   sample_draw_kernel    one workgroup per row: the chunk holding t (prefix of the kept masses in chunk order), then an in-order
//                         block scan of that chunk
// The mass is fixed point (w = exp(x - max) in [0, 1] as an integer w * 2^38, sums < 2^62 for V <= 2^24): integer atomics and
// integer sums give the same bits in any order, so the kept set and the drawn token are bitwise deterministic.  Hand-offs
// between workgroups go through launch boundaries only.
#include "mm_common.h"

namespace {

constexpr int SCHUNK = 4096;               // vocabulary entries per workgroup
constexpr int SPT = SCHUNK / 256;          // 16 contiguous entries per thread
constexpr int NB = 2048;                   // buckets of the widest digit
constexpr int MAXPASS = 6;                 // 3 digits x (top-k, top-p)
constexpr int MAXV = 1 << 24;
constexpr float WSCALE = 0x1p38f;
typedef unsigned long long u64;

struct SState {              // a row's selection after a pass (slot j = after pass j)
  unsigned prefix, mask;     // resolved high bits of the key being selected
  unsigned kr;               // top-k: the rank still to find inside the prefix group
  unsigned thr_k;            // top-k threshold key once resolved (0: every key)
  u64 above;                 // top-p: kept mass above the prefix group
  double target;             // top-p: top_p * Z_K
};

struct SArgs {
  const void* logits;
  int V, ld, C, vec;
  float temperature, min_p, top_p;
  int top_k, sel_k, npass;
  u64 seed, offset;
  int64_t* out;
  float* thresh;
  // workspace
  float* cmax;               // [rows, C]
  u64* cmass;                // [rows, C]
  unsigned* ckey;            // [rows, C]
  unsigned* hcnt;            // [rows, MAXPASS, NB]
  u64* hmass;                // [rows, MAXPASS, NB]
  SState* st;                // [rows, MAXPASS]
  unsigned* thr;             // [rows]
};

// order-preserving key: larger x <=> larger key (after -0 -> +0)
__device__ __forceinline__ unsigned fkey(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float kfloat(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
__device__ __forceinline__ int dshift(int d) { return d == 0 ? 21 : (d == 1 ? 10 : 0); }
__device__ __forceinline__ int dbuckets(int d) { return d == 2 ? 1024 : 2048; }
__device__ __forceinline__ u64 wfix(float w) { return w > 0.f ? (u64)(fminf(w, 1.f) * WSCALE) : 0ull; }   // NaN -> 0

// x[j] = float(logit[e0 + j]) / T (fp32 division), -0 -> +0; returns the number of valid entries (<= 0: none)
template <typename T>
__device__ __forceinline__ int load_x(const SArgs& a, int r, int c, float* x) {
  const T* row = (const T*)a.logits + (int64_t)r * a.ld;
  const int e0 = c * SCHUNK + (int)threadIdx.x * SPT;
  const int n = min(SPT, a.V - e0);
  if (a.vec && n == SPT) {
    constexpr int N = Vec16<T>::N;
    const Vec16<T>* p = (const Vec16<T>*)(row + e0);
#pragma unroll
    for (int i = 0; i < SPT / N; ++i) {
      const Vec16<T> v = p[i];
#pragma unroll
      for (int j = 0; j < N; ++j) x[i * N + j] = v.get(j);
    }
  } else {
#pragma unroll
    for (int j = 0; j < SPT; ++j) x[j] = j < n ? to_f32(row[e0 + j]) : 0.f;
  }
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    x[j] = x[j] / a.temperature;
    if (x[j] == 0.f) x[j] = 0.f;
  }
  return n;
}

__device__ __forceinline__ float row_max(const SArgs& a, int r, float* red) {
  float m = -INFINITY;
  for (int i = threadIdx.x; i < a.C; i += 256) m = fmaxf(m, a.cmax[(int64_t)r * a.C + i]);
  return block_max_256(m, red);
}

__device__ __forceinline__ unsigned shfl_up_u32(unsigned v, int d) { return (unsigned)__shfl_up((int)v, d, 64); }
__device__ __forceinline__ u64 shfl_up_u64(u64 v, int d) {
  return ((u64)shfl_up_u32((unsigned)(v >> 32), d) << 32) | shfl_up_u32((unsigned)v, d);
}

struct ScanLds {
  unsigned c[4];
  u64 m[4];
};
// exclusive scan of (c, m) over the 256 threads in thread order; totals of the block in ct, mt
__device__ __forceinline__ void block_excl_scan(unsigned& c, u64& m, unsigned& ct, u64& mt, ScanLds* s) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned ci = c;
  u64 mi = m;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned oc = shfl_up_u32(ci, d);
    const u64 om = shfl_up_u64(mi, d);
    if (lane >= d) { ci += oc; mi += om; }
  }
  __syncthreads();
  if (lane == 63) { s->c[w] = ci; s->m[w] = mi; }
  __syncthreads();
  unsigned cb = 0;
  u64 mb = 0;
  for (int i = 0; i < w; ++i) { cb += s->c[i]; mb += s->m[i]; }
  ct = s->c[0] + s->c[1] + s->c[2] + s->c[3];
  mt = s->m[0] + s->m[1] + s->m[2] + s->m[3];
  c = cb + ci - c;
  m = mb + mi - m;
}

__device__ __forceinline__ SState init_state(const SArgs& a) {
  SState s;
  s.prefix = s.mask = 0;
  s.kr = (unsigned)a.top_k;
  s.thr_k = 0;
  s.above = 0;
  s.target = 0.0;
  return s;
}

struct ResolveLds {
  ScanLds scan;
  unsigned found, above_c;
  u64 above_m;
};

// resolve pass j of row r from its histogram, starting from state s (every thread returns the same state)
__device__ SState resolve(const SArgs& a, int r, int j, SState s, ResolveLds* L) {
  const int d = j % 3, nb = dbuckets(d), per = nb / 256, shift = dshift(d);
  const bool isk = j < 3 * a.sel_k;
  const unsigned* hc = a.hcnt + ((int64_t)r * MAXPASS + j) * NB;
  const u64* hm = a.hmass + ((int64_t)r * MAXPASS + j) * NB;
  // thread t takes buckets nb-1-per*t down to nb-per*(t+1): thread order = descending key order
  unsigned cl[8];
  u64 ml[8];
  unsigned cs = 0;
  u64 ms = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int b = nb - 1 - per * (int)threadIdx.x - i;
    cl[i] = (i < per && isk) ? hc[b] : 0u;
    ml[i] = (i < per && !isk) ? hm[b] : 0ull;
    cs += cl[i];
    ms += ml[i];
  }
  unsigned ct;
  u64 mt;
  if (threadIdx.x == 0) { L->found = 0xFFFFFFFFu; L->above_c = 0; L->above_m = 0; }
  block_excl_scan(cs, ms, ct, mt, &L->scan);     // its barriers also publish L->found
  double target = s.target;
  if (!isk && d == 0) target = (double)a.top_p * (double)mt;   // Z_K: pass 0 of top-p sees the whole set top-k kept
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (i < per) {
      const unsigned b = (unsigned)(nb - 1 - per * (int)threadIdx.x - i);
      if (isk) {
        if (cs < s.kr && s.kr <= cs + cl[i]) { L->found = b; L->above_c = cs; }
      } else {
        if ((double)(s.above + ms) < target && target <= (double)(s.above + ms + ml[i])) { L->found = b; L->above_m = ms; }
      }
      cs += cl[i];
      ms += ml[i];
    }
  }
  __syncthreads();
  const unsigned found = L->found, above_c = L->above_c;
  const u64 above_m = L->above_m;
  __syncthreads();
  // not found only for rows outside the contract (no finite logit, NaN): bucket 0 keeps the whole group
  const unsigned b = found == 0xFFFFFFFFu ? 0u : found;
  SState n = s;
  n.prefix = s.prefix | (b << shift);
  n.mask = s.mask | ((unsigned)(nb - 1) << shift);
  if (isk) {
    n.kr = s.kr - above_c;
    if (d == 2) { n.thr_k = n.prefix; n.prefix = 0; n.mask = 0; }   // top-p (if on) starts its own passes
  } else {
    n.above = s.above + above_m;
    n.target = target;
  }
  return n;
}

// the state before pass j's histogram: pass j - 1 resolved (workgroup (0, r) stores it in slot j - 1 for later launches)
__device__ __forceinline__ SState state_before(const SArgs& a, int r, int j, ResolveLds* L) {
  if (j == 0) return init_state(a);
  const SState prev = j == 1 ? init_state(a) : a.st[(int64_t)r * MAXPASS + j - 2];
  const SState s = resolve(a, r, j - 1, prev, L);
  if (blockIdx.x == 0 && threadIdx.x == 0) a.st[(int64_t)r * MAXPASS + j - 1] = s;
  return s;
}

template <typename T>
__global__ __launch_bounds__(256) void sample_max_kernel(SArgs a) {
  __shared__ float red[4];
  const int c = blockIdx.x, r = blockIdx.y;
  float x[SPT];
  const int n = load_x<T>(a, r, c, x);
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < SPT; ++j)
    if (j < n) mx = fmaxf(mx, x[j]);
  mx = block_max_256(mx, red);
  if (threadIdx.x == 0) a.cmax[(int64_t)r * a.C + c] = mx;
  const int nz = a.npass * NB;
  unsigned* hc = a.hcnt + (int64_t)r * MAXPASS * NB;
  u64* hm = a.hmass + (int64_t)r * MAXPASS * NB;
  for (int i = c * 256 + (int)threadIdx.x; i < nz; i += a.C * 256) { hc[i] = 0u; hm[i] = 0ull; }
}

template <typename T>
__global__ __launch_bounds__(256) void sample_hist_kernel(SArgs a, int j) {
  __shared__ unsigned hc[NB];
  __shared__ u64 hm[NB];
  __shared__ float red[4];
  __shared__ ResolveLds L;
  const int c = blockIdx.x, r = blockIdx.y;
  for (int i = threadIdx.x; i < NB; i += 256) { hc[i] = 0u; hm[i] = 0ull; }
  const float m = row_max(a, r, red);
  const SState s = state_before(a, r, j, &L);
  const int d = j % 3, shift = dshift(d);
  const unsigned bmask = (unsigned)dbuckets(d) - 1u;
  const bool isk = j < 3 * a.sel_k;
  float x[SPT];
  const int n = load_x<T>(a, r, c, x);
  __syncthreads();                                  // LDS histogram zeroed
#pragma unroll
  for (int e = 0; e < SPT; ++e) {
    if (e < n) {
      const unsigned k = fkey(x[e]);
      if ((k & s.mask) == s.prefix && k >= s.thr_k) {
        const unsigned b = (k >> shift) & bmask;
        if (isk) {
          atomicAdd(&hc[b], 1u);
        } else {
          const u64 q = wfix(expf(x[e] - m));
          if (q) atomicAdd(&hm[b], q);
        }
      }
    }
  }
  __syncthreads();
  unsigned* gc = a.hcnt + ((int64_t)r * MAXPASS + j) * NB;
  u64* gm = a.hmass + ((int64_t)r * MAXPASS + j) * NB;
  for (int i = threadIdx.x; i <= (int)bmask; i += 256) {
    if (hc[i]) atomicAdd(gc + i, hc[i]);
    if (hm[i]) atomicAdd(gm + i, hm[i]);
  }
}

// kept <=> key >= threshold key and w >= min_p
template <typename T>
__global__ __launch_bounds__(256) void sample_mass_kernel(SArgs a) {
  __shared__ float red[4];
  __shared__ ResolveLds L;
  __shared__ unsigned kmin_w[4];
  const int c = blockIdx.x, r = blockIdx.y;
  const float m = row_max(a, r, red);
  unsigned thr = 0;
  if (a.npass > 0) {
    const SState s = state_before(a, r, a.npass, &L);     // resolves the last pass
    thr = a.npass > 3 * a.sel_k ? s.prefix : s.thr_k;
  }
  if (c == 0 && threadIdx.x == 0) a.thr[r] = thr;
  float x[SPT];
  const int n = load_x<T>(a, r, c, x);
  u64 ms = 0;
  unsigned kmin = 0xFFFFFFFFu;
#pragma unroll
  for (int e = 0; e < SPT; ++e) {
    if (e < n) {
      const unsigned k = fkey(x[e]);
      const float w = expf(x[e] - m);
      if (k >= thr && w >= a.min_p) {
        ms += wfix(w);
        kmin = min(kmin, k);
      }
    }
  }
  unsigned cz = 0, ct;
  u64 mt;
  block_excl_scan(cz, ms, ct, mt, &L.scan);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, o, 64));
  if ((threadIdx.x & 63) == 0) kmin_w[threadIdx.x >> 6] = kmin;
  __syncthreads();
  if (threadIdx.x == 0) {
    a.cmass[(int64_t)r * a.C + c] = mt;
    a.ckey[(int64_t)r * a.C + c] = min(min(kmin_w[0], kmin_w[1]), min(kmin_w[2], kmin_w[3]));
  }
}

__device__ __forceinline__ unsigned draw24(u64 seed, u64 offset, int r) { return philox4x32_10((u64)r, offset, seed).x >> 8; }

template <typename T>
__global__ __launch_bounds__(256) void sample_draw_kernel(SArgs a) {
  __shared__ float red[4];
  __shared__ ScanLds scan;
  __shared__ unsigned kmin_w[4];
  __shared__ int chunk;
  __shared__ u64 chunk_base;
  __shared__ int pick;
  const int r = blockIdx.x;
  const float m = row_max(a, r, red);
  const u64* cm = a.cmass + (int64_t)r * a.C;
  // Z and the smallest kept key over the chunks
  u64 z = 0;
  unsigned kmin = 0xFFFFFFFFu;
  for (int i = threadIdx.x; i < a.C; i += 256) { z += cm[i]; kmin = min(kmin, a.ckey[(int64_t)r * a.C + i]); }
  unsigned cz = 0, ct;
  u64 Z;
  block_excl_scan(cz, z, ct, Z, &scan);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, o, 64));
  if ((threadIdx.x & 63) == 0) kmin_w[threadIdx.x >> 6] = kmin;
  if (threadIdx.x == 0) { chunk = -1; chunk_base = 0; pick = -1; }
  __syncthreads();
  if (a.thresh && threadIdx.x == 0) {
    const unsigned k = min(min(kmin_w[0], kmin_w[1]), min(kmin_w[2], kmin_w[3]));
    a.thresh[r] = k == 0xFFFFFFFFu ? __uint_as_float(0x7FC00000u) : kfloat(k);
  }
  // t = u * Z with u = k24 * 2^-24; C(v) > t <=> C(v) > floor(t) for integer C
  const u64 k24 = draw24(a.seed, a.offset, r);
  const u64 t = (Z >> 24) * k24 + (((Z & 0xFFFFFFull) * k24) >> 24);
  // the chunk holding t: prefix of the kept masses in chunk order, 256 chunks at a time
  u64 base = 0;
  for (int i0 = 0; i0 < a.C; i0 += 256) {
    const int i = i0 + (int)threadIdx.x;
    u64 mi = i < a.C ? cm[i] : 0ull, pre = mi;
    unsigned c0 = 0, cz2;
    u64 tot;
    block_excl_scan(c0, pre, cz2, tot, &scan);
    if (i < a.C && base + pre <= t && t < base + pre + mi) { chunk = i; chunk_base = base + pre; }
    base += tot;
  }
  __syncthreads();
  const int c = chunk;
  if (c >= 0) {
    const u64 cb = chunk_base;
    const unsigned thr = a.thr[r];
    float x[SPT];
    const int n = load_x<T>(a, r, c, x);
    u64 q[SPT];
    u64 ms = 0;
#pragma unroll
    for (int e = 0; e < SPT; ++e) {
      q[e] = 0;
      if (e < n) {
        const float w = expf(x[e] - m);
        if (fkey(x[e]) >= thr && w >= a.min_p) q[e] = wfix(w);
      }
      ms += q[e];
    }
    unsigned c1 = 0, cz3;
    u64 tot;
    block_excl_scan(c1, ms, cz3, tot, &scan);
    u64 acc = cb + ms;
#pragma unroll
    for (int e = 0; e < SPT; ++e) {
      if (acc <= t && t < acc + q[e]) pick = c * SCHUNK + (int)threadIdx.x * SPT + e;
      acc += q[e];
    }
  }
  __syncthreads();
  // no crossing only for rows outside the contract (Z = 0: no finite logit); any index in [0, V) will do
  if (threadIdx.x == 0) a.out[r] = (pick >= 0 && pick < a.V) ? (int64_t)pick : 0;
}

__global__ void sample_uniforms_kernel(u64 seed, u64 offset, int rows, float* u) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < rows) u[r] = (float)draw24(seed, offset, r) * 0x1p-24f;
}

struct WsLayout {
  int64_t cmass, hmass, st, cmax, ckey, hcnt, thr, total;
};
WsLayout ws_layout(int rows, int V) {
  const int64_t C = (V + SCHUNK - 1) / SCHUNK, R = rows;
  auto up = [](int64_t b) { return (b + 15) / 16 * 16; };
  WsLayout L;
  L.cmass = 0;
  L.hmass = L.cmass + up(R * C * 8);
  L.st = L.hmass + up(R * MAXPASS * NB * 8);
  L.cmax = L.st + up(R * MAXPASS * (int64_t)sizeof(SState));
  L.ckey = L.cmax + up(R * C * 4);
  L.hcnt = L.ckey + up(R * C * 4);
  L.thr = L.hcnt + up(R * MAXPASS * NB * 4);
  L.total = L.thr + up(R * 4);
  return L;
}

template <typename T>
void launch_all(const SArgs& a, int rows, hipStream_t s) {
  const dim3 grid((unsigned)a.C, (unsigned)rows), block(256);
  hipLaunchKernelGGL(sample_max_kernel<T>, grid, block, 0, s, a);
  for (int j = 0; j < a.npass; ++j) hipLaunchKernelGGL(sample_hist_kernel<T>, grid, block, 0, s, a, j);
  hipLaunchKernelGGL(sample_mass_kernel<T>, grid, block, 0, s, a);
  hipLaunchKernelGGL(sample_draw_kernel<T>, dim3((unsigned)rows), block, 0, s, a);
}

}  // namespace

extern "C" int mm_sample_ws_bytes(int rows, int V, int64_t* bytes) {
  if (!bytes || rows < 0 || V <= 0 || V > MAXV) return MM_ERR_ARG;
  *bytes = ws_layout(rows, V).total;
  return MM_OK;
}

extern "C" int mm_sample(int dtype, const void* logits, int rows, int V, int ld, float temperature, int top_k, float top_p,
                         float min_p, int64_t seed, int64_t offset, int64_t* out, float* thresh, void* ws, int64_t ws_bytes,
                         void* stream) {
  if (dtype != MM_BF16 && dtype != MM_F32) return MM_ERR_ARG;
  if (!logits || !out || !ws || rows < 0 || V <= 0 || V > MAXV || ld < V) return MM_ERR_ARG;
  if (!(temperature > 0.f) || top_k < 0 || !(top_p > 0.f && top_p <= 1.f) || !(min_p >= 0.f && min_p <= 1.f)) return MM_ERR_ARG;
  const WsLayout L = ws_layout(rows, V);
  if (ws_bytes < L.total) return MM_ERR_ARG;
  if (((uintptr_t)ws) & 15) return MM_ERR_ALIGN;
  if (rows == 0) return MM_OK;
  char* w = (char*)ws;
  SArgs a;
  a.logits = logits;
  a.V = V;
  a.ld = ld;
  a.C = (V + SCHUNK - 1) / SCHUNK;
  a.vec = mm_aligned16(logits) && ((int64_t)ld * mm_elem_size(dtype)) % 16 == 0;
  a.temperature = temperature;
  a.min_p = min_p;
  a.top_p = top_p;
  a.top_k = top_k;
  a.sel_k = top_k > 0 && top_k < V;
  a.npass = 3 * (a.sel_k + (top_p < 1.f ? 1 : 0));
  a.seed = (u64)seed;
  a.offset = (u64)offset;
  a.out = out;
  a.thresh = thresh;
  a.cmass = (u64*)(w + L.cmass);
  a.hmass = (u64*)(w + L.hmass);
  a.st = (SState*)(w + L.st);
  a.cmax = (float*)(w + L.cmax);
  a.ckey = (unsigned*)(w + L.ckey);
  a.hcnt = (unsigned*)(w + L.hcnt);
  a.thr = (unsigned*)(w + L.thr);
  if (dtype == MM_BF16)
    launch_all<bf16>(a, rows, (hipStream_t)stream);
  else
    launch_all<float>(a, rows, (hipStream_t)stream);
  MM_CHECK_LAUNCH();
  return MM_OK;
}

extern "C" int mm_sample_uniforms(int64_t seed, int64_t offset, int rows, float* u, void* stream) {
  if (!u || rows < 0) return MM_ERR_ARG;
  if (rows == 0) return MM_OK;
  hipLaunchKernelGGL(sample_uniforms_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, (u64)seed, (u64)offset,
                     rows, u);
  MM_CHECK_LAUNCH();
  return MM_OK;
}
