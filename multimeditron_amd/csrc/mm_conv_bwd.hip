// Kernels for TRAINING the MoE gating network (model/modalities/gating.py): BatchNorm with batch statistics, forward and backward,
// and the max-pool's backward.  The contracts are written out in include/mm_hip.h; tests/conv_train_check.py restates them in fp64.
//
//   bn_stats_kernel       a workgroup owns BN_ROWS rows of a slab of 8 channel vectors: per channel its mean and the sum of squared
//                         deviations from THAT mean (two sweeps over rows it has just read), as fp32 partials
//   bn_finalize_kernel    one thread per channel merges the partials in row order (Chan, Golub & LeVeque 1979), writes mean / invstd
//                         and updates the running statistics
//   bn_apply_kernel       y = T(act(fma((z - mean) * invstd, gamma, beta) (+ residual))), one thread per 16-byte vector
//   bn_bwd_stats_kernel   the same slabs: sum g and sum g * xhat as fp32 partials
//   bn_bwd_finalize_kernel  sums the partials in order; dgamma / dbeta in T, the fp32 sums for the elementwise pass
//   bn_bwd_apply_kernel   dz (and dres) per 16-byte vector
//   maxpool_bwd_kernel    gather form: one thread per 16-byte channel vector of an INPUT pixel recomputes the argmax of the at most
//                         four windows that hold it
// Column sums: a thread adds every 32nd row of its slab (16 additions), the 32 row groups are added as a tree in LDS (5 levels),
// the workgroups in order.  No atomics anywhere.
#include "mm_common.h"

#include <limits.h>

namespace {

constexpr int BN_ROWS = 512;       // rows per workgroup
constexpr int BN_TV = 8;           // 16-byte channel vectors per workgroup (64 bf16 / 32 f32 channels)
constexpr int BN_TR = 32;          // row groups per workgroup (256 threads)

// tree sum of v[N] over the BN_TR row groups of the workgroup; every thread returns with the totals of its channel vector
template <int N>
__device__ __forceinline__ void slab_sum(float (&v)[N], float* red, int tr, int tv) {
  __syncthreads();                                                 // red may still be read from the previous sum
#pragma unroll
  for (int j = 0; j < N; ++j) red[(tr * BN_TV + tv) * N + j] = v[j];
#pragma unroll
  for (int o = BN_TR / 2; o > 0; o >>= 1) {
    __syncthreads();
    if (tr < o) {
#pragma unroll
      for (int j = 0; j < N; ++j) red[(tr * BN_TV + tv) * N + j] += red[((tr + o) * BN_TV + tv) * N + j];
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < N; ++j) v[j] = red[tv * N + j];
}

template <typename T>
__global__ __launch_bounds__(256) void bn_stats_kernel(const T* __restrict__ z, int M, int C, float* __restrict__ partial) {
  constexpr int N = Vec16<T>::N;
  __shared__ float red[BN_TR * BN_TV * N];
  const int tv = threadIdx.x & (BN_TV - 1), tr = threadIdx.x / BN_TV;
  const int c = (blockIdx.x * BN_TV + tv) * N;
  const int row0 = blockIdx.y * BN_ROWS;
  const int rows = min(BN_ROWS, M - row0);
  const T* zb = z + (int64_t)row0 * C + c;
  float s[N];
#pragma unroll
  for (int j = 0; j < N; ++j) s[j] = 0.f;
  for (int r = tr; r < rows; r += BN_TR) {
    const Vec16<T> v = *(const Vec16<T>*)(zb + (int64_t)r * C);
#pragma unroll
    for (int j = 0; j < N; ++j) s[j] += v.get(j);
  }
  slab_sum<N>(s, red, tr, tv);
  float mu[N], q[N];
#pragma unroll
  for (int j = 0; j < N; ++j) { mu[j] = s[j] / (float)rows; q[j] = 0.f; }
  for (int r = tr; r < rows; r += BN_TR) {
    const Vec16<T> v = *(const Vec16<T>*)(zb + (int64_t)r * C);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const float d = v.get(j) - mu[j];
      q[j] = __builtin_fmaf(d, d, q[j]);
    }
  }
  slab_sum<N>(q, red, tr, tv);
  if (tr == 0) {
    float* p = partial + (int64_t)blockIdx.y * 2 * C + c;
#pragma unroll
    for (int j = 0; j < N; ++j) { p[j] = mu[j]; p[C + j] = q[j]; }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ partial, int nsplit, int M, int C, float eps,
                                                          float momentum, float* __restrict__ mean, float* __restrict__ invstd,
                                                          T* __restrict__ rmean, T* __restrict__ rvar, int64_t* __restrict__ nbt) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float na = 0.f, mu = 0.f, m2 = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float nb = (float)min(BN_ROWS, M - s * BN_ROWS);
    const float mb = partial[(int64_t)s * 2 * C + c], qb = partial[(int64_t)s * 2 * C + C + c];
    const float nab = na + nb, delta = mb - mu;
    mu += delta * (nb / nab);
    m2 += qb + delta * delta * (na * nb / nab);
    na = nab;
  }
  mean[c] = mu;
  invstd[c] = 1.f / sqrtf(m2 / (float)M + eps);
  if (rmean) {
    rmean[c] = from_f32<T>((1.f - momentum) * to_f32(rmean[c]) + momentum * mu);
    rvar[c] = from_f32<T>((1.f - momentum) * to_f32(rvar[c]) + momentum * (m2 / (float)(M - 1)));
    if (c == 0) nbt[0] += 1;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ z, int64_t total, int C, const float* __restrict__ mean,
                                                       const float* __restrict__ invstd, const T* __restrict__ gamma,
                                                       const T* __restrict__ beta, const T* __restrict__ res, int relu,
                                                       T* __restrict__ y) {
  constexpr int N = Vec16<T>::N;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;       // (row, channel vector)
  if (i >= total) return;
  const int c = (int)(i % (C / N)) * N;
  const Vec16<T> zv = *(const Vec16<T>*)(z + i * N);
  const Vec16<T> gv = *(const Vec16<T>*)(gamma + c), bv = *(const Vec16<T>*)(beta + c);
  Vec16<T> rv, o;
  if (res) rv = *(const Vec16<T>*)(res + i * N);
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const float xhat = (zv.get(j) - mean[c + j]) * invstd[c + j];
    float v = __builtin_fmaf(xhat, gv.get(j), bv.get(j));
    if (res) v += rv.get(j);
    if (relu) v = fmaxf(v, 0.f);
    o.set(j, v);
  }
  *(Vec16<T>*)(y + i * N) = o;
}

template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_stats_kernel(const T* __restrict__ dy, const T* __restrict__ y, const T* __restrict__ z,
                                                           int M, int C, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, int relu, float* __restrict__ partial) {
  constexpr int N = Vec16<T>::N;
  __shared__ float red[BN_TR * BN_TV * N];
  const int tv = threadIdx.x & (BN_TV - 1), tr = threadIdx.x / BN_TV;
  const int c = (blockIdx.x * BN_TV + tv) * N;
  const int row0 = blockIdx.y * BN_ROWS;
  const int rows = min(BN_ROWS, M - row0);
  const int64_t base = (int64_t)row0 * C + c;
  float mu[N], is[N], s1[N], s2[N];
#pragma unroll
  for (int j = 0; j < N; ++j) { mu[j] = mean[c + j]; is[j] = invstd[c + j]; s1[j] = s2[j] = 0.f; }
  for (int r = tr; r < rows; r += BN_TR) {
    const int64_t at = base + (int64_t)r * C;
    const Vec16<T> dv = *(const Vec16<T>*)(dy + at), zv = *(const Vec16<T>*)(z + at);
    Vec16<T> yv;
    if (relu) yv = *(const Vec16<T>*)(y + at);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const float g = (!relu || yv.get(j) > 0.f) ? dv.get(j) : 0.f;
      const float xhat = (zv.get(j) - mu[j]) * is[j];
      s1[j] += g;
      s2[j] = __builtin_fmaf(g, xhat, s2[j]);
    }
  }
  slab_sum<N>(s1, red, tr, tv);
  slab_sum<N>(s2, red, tr, tv);
  if (tr == 0) {
    float* p = partial + (int64_t)blockIdx.y * 2 * C + c;
#pragma unroll
    for (int j = 0; j < N; ++j) { p[j] = s1[j]; p[C + j] = s2[j]; }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* __restrict__ partial, int nsplit, int C,
                                                              float* __restrict__ sums, T* __restrict__ dgamma, T* __restrict__ dbeta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s1 = 0.f, s2 = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    s1 += partial[(int64_t)s * 2 * C + c];
    s2 += partial[(int64_t)s * 2 * C + C + c];
  }
  sums[c] = s1;
  sums[C + c] = s2;
  dbeta[c] = from_f32<T>(s1);
  dgamma[c] = from_f32<T>(s2);
}

template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ dy, const T* __restrict__ y, const T* __restrict__ z,
                                                           int64_t total, int C, float invM, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const T* __restrict__ gamma,
                                                           const float* __restrict__ sums, int relu, T* __restrict__ dz,
                                                           T* __restrict__ dres) {
  constexpr int N = Vec16<T>::N;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % (C / N)) * N;
  const Vec16<T> dv = *(const Vec16<T>*)(dy + i * N), zv = *(const Vec16<T>*)(z + i * N), gv = *(const Vec16<T>*)(gamma + c);
  Vec16<T> yv, o, r;
  if (relu) yv = *(const Vec16<T>*)(y + i * N);
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const float g = (!relu || yv.get(j) > 0.f) ? dv.get(j) : 0.f;
    const float is = invstd[c + j];
    const float xhat = (zv.get(j) - mean[c + j]) * is;
    o.set(j, gv.get(j) * is * (g - sums[c + j] * invM - xhat * (sums[C + c + j] * invM)));
    r.set(j, g);
  }
  *(Vec16<T>*)(dz + i * N) = o;
  if (dres) *(Vec16<T>*)(dres + i * N) = r;
}

template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy, int H, int W, int C,
                                                          int Ho, int Wo, int64_t total, T* __restrict__ dx) {
  constexpr int N = Vec16<T>::N;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // (image, h, w, channel vector) of the INPUT
  if (i >= total) return;
  const int cv = C / N;
  const int v = (int)(i % cv);
  int64_t t = i / cv;
  const int w = (int)(t % W);
  t /= W;
  const int h = (int)(t % H);
  const int64_t img = t / H;
  float acc[N];
#pragma unroll
  for (int j = 0; j < N; ++j) acc[j] = 0.f;
  // the windows that hold (h, w): 2 ho - 1 <= h <= 2 ho + 1
  const int ho_lo = h / 2, ho_hi = min((h + 1) / 2, Ho - 1);
  const int wo_lo = w / 2, wo_hi = min((w + 1) / 2, Wo - 1);
  for (int ho = ho_lo; ho <= ho_hi; ++ho) {
    for (int wo = wo_lo; wo <= wo_hi; ++wo) {
      const int mine = (h - (2 * ho - 1)) * 3 + (w - (2 * wo - 1));
      float best[N];
      int bi[N];
#pragma unroll
      for (int j = 0; j < N; ++j) { best[j] = -INFINITY; bi[j] = -1; }
#pragma unroll
      for (int dr = 0; dr < 3; ++dr) {
        const int hi = 2 * ho - 1 + dr;
        if ((unsigned)hi >= (unsigned)H) continue;                 // padding taps never win
#pragma unroll
        for (int ds = 0; ds < 3; ++ds) {
          const int wi = 2 * wo - 1 + ds;
          if ((unsigned)wi >= (unsigned)W) continue;
          const Vec16<T> xv = *(const Vec16<T>*)(x + ((img * H + hi) * W + wi) * C + (int64_t)v * N);
#pragma unroll
          for (int j = 0; j < N; ++j) {
            const float xj = xv.get(j);
            if (bi[j] < 0 || xj > best[j]) { best[j] = xj; bi[j] = dr * 3 + ds; }      // strict: the FIRST maximal element stays
          }
        }
      }
      const Vec16<T> dv = *(const Vec16<T>*)(dy + ((img * Ho + ho) * Wo + wo) * C + (int64_t)v * N);
#pragma unroll
      for (int j = 0; j < N; ++j)
        if (bi[j] == mine) acc[j] += dv.get(j);
    }
  }
  Vec16<T> o;
#pragma unroll
  for (int j = 0; j < N; ++j) o.set(j, acc[j]);
  *(Vec16<T>*)(dx + i * N) = o;
}

// ---------------------------------------------------------------- convolution gradients
struct ConvGradArgs {
  const void* dz;     // [n, Ho, Wo, Cout]
  const void* x;      // wgrad: [n, H, W, Cin]
  const void* w;      // dgrad: the filter packed [Cin, R, S, Cout]
  const void* add;    // dgrad: optional addend [n, H, W, Cin]
  void* out;          // dgrad: dx [n, H, W, Cin]
  float* partial;     // wgrad: [nsplit, Cout, K] fp32
  int H, W, Cin, Ho, Wo, Cout, R, stride, pad;
  int M;              // dgrad: n * H * W input pixels; wgrad: n * Ho * Wo output pixels
  int K;              // dgrad: R * R * Cout; wgrad: R * R * Cin
  int rows;           // wgrad: output pixels per M split (a multiple of 32)
};

// dgrad: the gather form of conv_bf16_kernel (mm_conv.hip).  D^T[cin, pixel] = Wp[cin, k] . dZ[k, pixel], k = (r * S + s) * Cout + cout:
// the 8 k-values of one lane are 8 contiguous output channels of ONE tap, so both fragments are one 16-byte load.  Tap (r, s) of input
// pixel (h, w) reads output pixel ((h + pad - r) / stride, (w + pad - s) / stride) when both divisions are exact and the result lies in
// the image; otherwise the fragment is zero and nothing is loaded.  One wave owns 64 cins x 32 input pixels.
__global__ __launch_bounds__(256) void dgrad_bf16_kernel(const ConvGradArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int m_wave = (blockIdx.x * 4 + wave) * 32;
  if (m_wave >= a.M) return;                                       // wave-uniform
  const int m = m_wave + r;
  const bool mv = m < a.M;
  const int ci0 = blockIdx.y * 64;
  int hp = 0, wp_ = 0;
  const bf16* zb = (const bf16*)a.dz;
  if (mv) {
    const int wi = m % a.W, t = m / a.W, hi = t % a.H, img = t / a.H;
    hp = hi + a.pad;
    wp_ = wi + a.pad;
    zb += (int64_t)img * a.Ho * a.Wo * a.Cout;
  }
  const bf16* w0 = (const bf16*)a.w + (int64_t)(ci0 + r) * a.K;
  const bf16* w1 = w0 + (int64_t)32 * a.K;
  const int cg = a.Cout >> 3, KG = a.K >> 3;
  int tap = h / cg, c8 = h - tap * cg;
  int rr = tap / a.R, ss = tap - rr * a.R;
  f32x16 acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int g = h; g - h < KG; g += 2) {
    bf16x8 fa0 = zero, fa1 = zero, fb = zero;
    if (g < KG) {
      fa0 = *(const bf16x8*)(w0 + g * 8);
      fa1 = *(const bf16x8*)(w1 + g * 8);
      const int hn = hp - rr, wn = wp_ - ss;                       // stride * ho, stride * wo
      if (mv && hn >= 0 && wn >= 0 && !(hn & (a.stride - 1)) && !(wn & (a.stride - 1))) {
        const int ho = hn >> (a.stride - 1), wo = wn >> (a.stride - 1);      // stride is 1 or 2
        if (ho < a.Ho && wo < a.Wo) fb = *(const bf16x8*)(zb + ((int64_t)ho * a.Wo + wo) * a.Cout + c8 * 8);
      }
    }
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa0, fb, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa1, fb, acc1, 0, 0, 0);
    c8 += 2;
    while (c8 >= cg) {
      c8 -= cg;
      if (++ss == a.R) { ss = 0; ++rr; }
    }
  }
  if (!mv) return;
  bf16* orow = (bf16*)a.out + (int64_t)m * a.Cin;
  const bf16* arow = a.add ? (const bf16*)a.add + (int64_t)m * a.Cin : nullptr;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ci = ci0 + 32 * t + 8 * q + 4 * h;
      bf16x4 av = {0, 0, 0, 0};
      if (arow) av = *(const bf16x4*)(arow + ci);
      bf16x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v = t ? acc1[4 * q + j] : acc0[4 * q + j];
        if (arow) v += (float)av[j];
        o[j] = (bf16)v;
      }
      *(bf16x4*)(orow + ci) = o;
    }
  }
}

__global__ __launch_bounds__(256) void dgrad_f32_kernel(const ConvGradArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)a.M * a.Cin) return;
  const int ci = (int)(idx % a.Cin), m = (int)(idx / a.Cin);
  const int wi = m % a.W, t = m / a.W, hi = t % a.H, img = t / a.H;
  const float* zb = (const float*)a.dz + (int64_t)img * a.Ho * a.Wo * a.Cout;
  const float* wb = (const float*)a.w + (int64_t)ci * a.K;
  float acc = 0.f;
  for (int rr = 0; rr < a.R; ++rr) {
    const int hn = hi + a.pad - rr;
    if (hn < 0 || (hn & (a.stride - 1)) || (hn >> (a.stride - 1)) >= a.Ho) continue;
    for (int ss = 0; ss < a.R; ++ss) {
      const int wn = wi + a.pad - ss;
      if (wn < 0 || (wn & (a.stride - 1)) || (wn >> (a.stride - 1)) >= a.Wo) continue;
      const f32x4* zp = (const f32x4*)(zb + ((int64_t)(hn >> (a.stride - 1)) * a.Wo + (wn >> (a.stride - 1))) * a.Cout);
      const f32x4* wq = (const f32x4*)(wb + (int64_t)(rr * a.R + ss) * a.Cout);
      f32x4 part = {0.f, 0.f, 0.f, 0.f};
      for (int c = 0; c < a.Cout / 4; ++c) {
        const f32x4 zv = zp[c], wv = wq[c];
#pragma unroll
        for (int j = 0; j < 4; ++j) part[j] = __builtin_fmaf(zv[j], wv[j], part[j]);
      }
      acc += (part[0] + part[1]) + (part[2] + part[3]);
    }
  }
  if (a.add) acc += ((const float*)a.add)[idx];
  ((float*)a.out)[idx] = acc;
}

// wgrad: dW[cout, kk] = sum_m dZ[m, cout] * X[m @ tap(kk), cin(kk)], kk = (r * S + s) * Cin + cin.  The sum runs over pixels, the strided
// dimension of both operands, so both MFMA fragments (8 consecutive m of ONE channel per lane) are transposed reads: a workgroup
// stages 32 pixels x 64 couts of dZ and 32 pixels x 64 kk of X (a tap outside the image, a pixel past the split or a kk past K as
// zeros) in LDS by rows and reads them with ds_read_b64_tr_b16.  Rows are 192 bytes apart (128 of data): the four rows one 32-lane
// half reads then start at banks 0, 48, 32, 16 and never meet.  Wave w owns couts 32 (w & 1) and kk 32 (w >> 1) of the 64 x 64 tile;
// blockIdx.z is the M split, whose fp32 tile goes to its own slice of the workspace.
constexpr int WG_ROWB = 192;       // bytes between LDS rows

__global__ __launch_bounds__(256) void wgrad_bf16_kernel(const ConvGradArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[2 * 32 * WG_ROWB];
  char* lz = lds;
  char* lx = lds + 32 * WG_ROWB;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kk0 = blockIdx.x * 64, co0 = blockIdx.y * 64;
  const int m_lo = blockIdx.z * a.rows, m_hi = min(a.M, m_lo + a.rows);
  // loader: thread -> (row, 16-byte chunk)
  const int lrow = threadIdx.x >> 3, lch = threadIdx.x & 7;
  const int kk = kk0 + lch * 8;
  const bool kv = kk < a.K;
  const int tap = kv ? kk / a.Cin : 0, cin = kv ? kk - tap * a.Cin : 0;
  const int rr = tap / a.R, ss = tap - rr * a.R;
  const bf16* zg = (const bf16*)a.dz + co0 + lch * 8;
  const bf16* xg = (const bf16*)a.x + cin;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  // transposed reads: lane 4q + p of a 16-lane group supplies row q, columns 4p .. 4p+3 of the group's 4 x 16 block
  const int i16 = lane & 15, g = lane >> 4;
  const int tr_row = 8 * (g >> 1) + (i16 >> 2), tr_col = 16 * (g & 1) + 4 * (i16 & 3);
  const int za = tr_row * WG_ROWB + (32 * (wave & 1) + tr_col) * 2;
  const int xa = tr_row * WG_ROWB + (32 * (wave >> 1) + tr_col) * 2;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  bf16x8 rz = zero, rx = zero;
  auto load = [&](int m0) {
    const int m = m0 + lrow;
    rz = zero;
    rx = zero;
    if (m < m_hi) {
      rz = *(const bf16x8*)(zg + (int64_t)m * a.Cout);
      const int wo = m % a.Wo, t = m / a.Wo, ho = t % a.Ho, img = t / a.Ho;
      const int hi = ho * a.stride - a.pad + rr, wi = wo * a.stride - a.pad + ss;
      if (kv && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W)
        rx = *(const bf16x8*)(xg + (((int64_t)img * a.H + hi) * a.W + wi) * a.Cin);
    }
  };
  load(m_lo);
  for (int m0 = m_lo; m0 < m_hi; m0 += 32) {                        // uniform over the workgroup: every lane reaches the reads below
    __syncthreads();
    *(bf16x8*)(lz + lrow * WG_ROWB + lch * 16) = rz;
    *(bf16x8*)(lx + lrow * WG_ROWB + lch * 16) = rx;
    __syncthreads();
    if (m0 + 32 < m_hi) load(m0 + 32);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(LDS_PTR(bf16x4, lz + za + (16 * ks) * WG_ROWB));
      const bf16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(LDS_PTR(bf16x4, lz + za + (16 * ks + 4) * WG_ROWB));
      const bf16x4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(LDS_PTR(bf16x4, lx + xa + (16 * ks) * WG_ROWB));
      const bf16x4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(LDS_PTR(bf16x4, lx + xa + (16 * ks + 4) * WG_ROWB));
      const bf16x8 fa = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
      const bf16x8 fb = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc, 0, 0, 0);
    }
  }
  // accumulator register i: cout = (i & 3) + 8 (i >> 2) + 4 h, kk = this lane's
  const int r = lane & 31, h = lane >> 5;
  const int okk = kk0 + 32 * (wave >> 1) + r;
  if (okk < a.K) {
    float* p = a.partial + ((int64_t)blockIdx.z * a.Cout + co0 + 32 * (wave & 1)) * a.K + okk;
#pragma unroll
    for (int i = 0; i < 16; ++i) p[(int64_t)((i & 3) + 8 * (i >> 2) + 4 * h) * a.K] = acc[i];
  }
}

__global__ __launch_bounds__(256) void wgrad_f32_kernel(const ConvGradArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;      // (cout, kk)
  if (idx >= (int64_t)a.Cout * a.K) return;
  const int kk = (int)(idx % a.K), co = (int)(idx / a.K);
  const int tap = kk / a.Cin, cin = kk - tap * a.Cin;
  const int rr = tap / a.R, ss = tap - rr * a.R;
  const int m_lo = blockIdx.y * a.rows, m_hi = min(a.M, m_lo + a.rows);
  const float* zg = (const float*)a.dz + co;
  const float* xg = (const float*)a.x + cin;
  float acc = 0.f;
  for (int m = m_lo; m < m_hi; ++m) {
    const int wo = m % a.Wo, t = m / a.Wo, ho = t % a.Ho, img = t / a.Ho;
    const int hi = ho * a.stride - a.pad + rr, wi = wo * a.stride - a.pad + ss;
    if ((unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W)
      acc = __builtin_fmaf(zg[(int64_t)m * a.Cout], xg[(((int64_t)img * a.H + hi) * a.W + wi) * a.Cin], acc);
  }
  a.partial[(int64_t)blockIdx.y * a.Cout * a.K + idx] = acc;
}

constexpr int WG_SPLIT_ROWS = 1024;    // output pixels per M split of the weight gradient
int64_t wgrad_nsplit(int64_t M) { return M <= 0 ? 1 : (M + WG_SPLIT_ROWS - 1) / WG_SPLIT_ROWS; }

// the checks the two convolution gradients share (the forward's rules); fills Ho / Wo
int conv_grad_check(int dtype, int n, int H, int W, int Cin, int Cout, int R, int stride, int pad, int* Ho, int* Wo) {
  if (n < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || pad < 0) return MM_ERR_ARG;
  if (dtype != MM_BF16 && dtype != MM_F32) return MM_ERR_UNSUPPORTED;
  if ((R != 1 && R != 3 && R != 7) || (stride != 1 && stride != 2) || (pad != 0 && pad != 1 && pad != 3)) return MM_ERR_UNSUPPORTED;
  if (H + 2 * pad < R || W + 2 * pad < R) return MM_ERR_ARG;
  *Ho = (H + 2 * pad - R) / stride + 1;
  *Wo = (W + 2 * pad - R) / stride + 1;
  return MM_OK;
}

int64_t bn_nsplit(int M) { return ((int64_t)M + BN_ROWS - 1) / BN_ROWS; }
int64_t bn_ws_bytes(int M, int C) { return (2 * bn_nsplit(M) + 2) * (int64_t)C * 4; }

// the checks the two BatchNorm entry points share; MM_OK when a launch may follow
int bn_check(int dtype, int M, int C, const void* ws, int64_t ws_bytes) {
  if (M < 2 || C <= 0 || !ws) return MM_ERR_ARG;
  if (dtype != MM_BF16 && dtype != MM_F32) return MM_ERR_UNSUPPORTED;
  if ((C % 64) || !mm_aligned16(ws)) return MM_ERR_ALIGN;
  if (ws_bytes < bn_ws_bytes(M, C)) return MM_ERR_ARG;
  const int vn = dtype == MM_BF16 ? 8 : 4;
  if (bn_nsplit(M) > 65535 || ((int64_t)M * (C / vn) + 255) / 256 > INT_MAX) return MM_ERR_UNSUPPORTED;
  return MM_OK;
}

}  // namespace

extern "C" int mm_bn_train_ws_bytes(int M, int C, int64_t* bytes) {
  if (!bytes || M < 2 || C <= 0) return MM_ERR_ARG;
  *bytes = bn_ws_bytes(M, C);
  return MM_OK;
}

extern "C" int mm_bn_train_fwd(int dtype, const void* z, int M, int C, const void* gamma, const void* beta, const void* residual,
                               int relu, float eps, float momentum, void* y, float* mean, float* invstd, void* running_mean,
                               void* running_var, int64_t* num_batches_tracked, void* ws, int64_t ws_bytes, void* stream) {
  if (!z || !gamma || !beta || !y || !mean || !invstd || !(eps > 0.f) || !(momentum >= 0.f && momentum <= 1.f)) return MM_ERR_ARG;
  const int all = (running_mean != nullptr) + (running_var != nullptr) + (num_batches_tracked != nullptr);
  if (all != 0 && all != 3) return MM_ERR_ARG;
  const int rc = bn_check(dtype, M, C, ws, ws_bytes);
  if (rc != MM_OK) return rc;
  if (!mm_aligned16(z) || !mm_aligned16(y) || !mm_aligned16(gamma) || !mm_aligned16(beta) || (residual && !mm_aligned16(residual)) ||
      (running_mean && (!mm_aligned16(running_mean) || !mm_aligned16(running_var))))
    return MM_ERR_ALIGN;
  const int vn = dtype == MM_BF16 ? 8 : 4;
  const int nsplit = (int)bn_nsplit(M);
  const int64_t total = (int64_t)M * (C / vn);
  float* partial = (float*)ws;
  hipStream_t s = (hipStream_t)stream;
  dim3 sgrid((unsigned)(C / (BN_TV * vn)), (unsigned)nsplit), block(256), cgrid((unsigned)((C + 255) / 256)),
      egrid((unsigned)((total + 255) / 256));
  if (dtype == MM_BF16) {
    hipLaunchKernelGGL(bn_stats_kernel<bf16>, sgrid, block, 0, s, (const bf16*)z, M, C, partial);
    hipLaunchKernelGGL(bn_finalize_kernel<bf16>, cgrid, block, 0, s, partial, nsplit, M, C, eps, momentum, mean, invstd,
                       (bf16*)running_mean, (bf16*)running_var, num_batches_tracked);
    hipLaunchKernelGGL(bn_apply_kernel<bf16>, egrid, block, 0, s, (const bf16*)z, total, C, mean, invstd, (const bf16*)gamma,
                       (const bf16*)beta, (const bf16*)residual, relu ? 1 : 0, (bf16*)y);
  } else {
    hipLaunchKernelGGL(bn_stats_kernel<float>, sgrid, block, 0, s, (const float*)z, M, C, partial);
    hipLaunchKernelGGL(bn_finalize_kernel<float>, cgrid, block, 0, s, partial, nsplit, M, C, eps, momentum, mean, invstd,
                       (float*)running_mean, (float*)running_var, num_batches_tracked);
    hipLaunchKernelGGL(bn_apply_kernel<float>, egrid, block, 0, s, (const float*)z, total, C, mean, invstd, (const float*)gamma,
                       (const float*)beta, (const float*)residual, relu ? 1 : 0, (float*)y);
  }
  MM_CHECK_LAUNCH();
  return MM_OK;
}

extern "C" int mm_bn_train_bwd(int dtype, const void* dy, const void* y, const void* z, int M, int C, const float* mean,
                               const float* invstd, const void* gamma, int relu, void* dz, void* dres, void* dgamma, void* dbeta,
                               void* ws, int64_t ws_bytes, void* stream) {
  if (!dy || !z || !mean || !invstd || !gamma || !dz || !dgamma || !dbeta || (relu && !y)) return MM_ERR_ARG;
  const int rc = bn_check(dtype, M, C, ws, ws_bytes);
  if (rc != MM_OK) return rc;
  if (!mm_aligned16(dy) || !mm_aligned16(z) || !mm_aligned16(gamma) || !mm_aligned16(dz) || (y && !mm_aligned16(y)) ||
      (dres && !mm_aligned16(dres)))
    return MM_ERR_ALIGN;
  const int vn = dtype == MM_BF16 ? 8 : 4;
  const int nsplit = (int)bn_nsplit(M);
  const int64_t total = (int64_t)M * (C / vn);
  float* partial = (float*)ws;
  float* sums = partial + (int64_t)2 * nsplit * C;
  const float invM = 1.f / (float)M;
  hipStream_t s = (hipStream_t)stream;
  dim3 sgrid((unsigned)(C / (BN_TV * vn)), (unsigned)nsplit), block(256), cgrid((unsigned)((C + 255) / 256)),
      egrid((unsigned)((total + 255) / 256));
  if (dtype == MM_BF16) {
    hipLaunchKernelGGL(bn_bwd_stats_kernel<bf16>, sgrid, block, 0, s, (const bf16*)dy, (const bf16*)y, (const bf16*)z, M, C, mean, invstd,
                       relu ? 1 : 0, partial);
    hipLaunchKernelGGL(bn_bwd_finalize_kernel<bf16>, cgrid, block, 0, s, partial, nsplit, C, sums, (bf16*)dgamma, (bf16*)dbeta);
    hipLaunchKernelGGL(bn_bwd_apply_kernel<bf16>, egrid, block, 0, s, (const bf16*)dy, (const bf16*)y, (const bf16*)z, total, C, invM, mean,
                       invstd, (const bf16*)gamma, sums, relu ? 1 : 0, (bf16*)dz, (bf16*)dres);
  } else {
    hipLaunchKernelGGL(bn_bwd_stats_kernel<float>, sgrid, block, 0, s, (const float*)dy, (const float*)y, (const float*)z, M, C, mean,
                       invstd, relu ? 1 : 0, partial);
    hipLaunchKernelGGL(bn_bwd_finalize_kernel<float>, cgrid, block, 0, s, partial, nsplit, C, sums, (float*)dgamma, (float*)dbeta);
    hipLaunchKernelGGL(bn_bwd_apply_kernel<float>, egrid, block, 0, s, (const float*)dy, (const float*)y, (const float*)z, total, C, invM,
                       mean, invstd, (const float*)gamma, sums, relu ? 1 : 0, (float*)dz, (float*)dres);
  }
  MM_CHECK_LAUNCH();
  return MM_OK;
}

extern "C" int mm_maxpool2d_nhwc_bwd(int dtype, const void* x, const void* dy, int n, int H, int W, int C, void* dx, void* stream) {
  if (!x || !dy || !dx || n < 0 || H <= 0 || W <= 0 || C <= 0) return MM_ERR_ARG;
  if (dtype != MM_BF16 && dtype != MM_F32) return MM_ERR_UNSUPPORTED;
  const int vn = dtype == MM_BF16 ? 8 : 4;
  if ((C % vn) || !mm_aligned16(x) || !mm_aligned16(dy) || !mm_aligned16(dx)) return MM_ERR_ALIGN;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const int64_t total = (int64_t)n * H * W * (C / vn);
  if (total == 0) return MM_OK;
  if ((total + 255) / 256 > INT_MAX) return MM_ERR_UNSUPPORTED;
  dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MM_BF16)
    hipLaunchKernelGGL(maxpool_bwd_kernel<bf16>, grid, block, 0, s, (const bf16*)x, (const bf16*)dy, H, W, C, Ho, Wo, total, (bf16*)dx);
  else
    hipLaunchKernelGGL(maxpool_bwd_kernel<float>, grid, block, 0, s, (const float*)x, (const float*)dy, H, W, C, Ho, Wo, total,
                       (float*)dx);
  MM_CHECK_LAUNCH();
  return MM_OK;
}

extern "C" int mm_conv2d_nhwc_dgrad(int dtype, const void* dz, int n, int H, int W, int Cin, const void* wp, int Cout, int R, int stride,
                                    int pad, const void* addend, void* dx, void* stream) {
  if (!dz || !wp || !dx) return MM_ERR_ARG;
  int Ho = 0, Wo = 0;
  const int rc = conv_grad_check(dtype, n, H, W, Cin, Cout, R, stride, pad, &Ho, &Wo);
  if (rc != MM_OK) return rc;
  if (R == 7) return MM_ERR_UNSUPPORTED;                           // the stem needs no data gradient
  if ((Cin % 64) || (Cout % 8)) return MM_ERR_ALIGN;
  if (!mm_aligned16(dz) || !mm_aligned16(wp) || !mm_aligned16(dx) || (addend && !mm_aligned16(addend))) return MM_ERR_ALIGN;
  const int64_t M = (int64_t)n * H * W, K = (int64_t)R * R * Cout, Mo = (int64_t)n * Ho * Wo;
  if (M > INT_MAX - 256 || Mo > INT_MAX - 256 || (int64_t)Cin * K > INT_MAX || M * Cin / 256 > INT_MAX - 1) return MM_ERR_UNSUPPORTED;
  if (M == 0) return MM_OK;
  ConvGradArgs a{dz, nullptr, wp, addend, dx, nullptr, H, W, Cin, Ho, Wo, Cout, R, stride, pad, (int)M, (int)K, 0};
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MM_BF16) {
    dim3 grid((unsigned)((M + 127) / 128), (unsigned)(Cin / 64)), block(256);
    hipLaunchKernelGGL(dgrad_bf16_kernel, grid, block, 0, s, a);
  } else {
    dim3 grid((unsigned)((M * Cin + 255) / 256)), block(256);
    hipLaunchKernelGGL(dgrad_f32_kernel, grid, block, 0, s, a);
  }
  MM_CHECK_LAUNCH();
  return MM_OK;
}

extern "C" int mm_conv2d_nhwc_wgrad_ws_bytes(int n, int H, int W, int Cin, int Cout, int R, int stride, int pad, int64_t* bytes) {
  if (!bytes) return MM_ERR_ARG;
  int Ho = 0, Wo = 0;
  const int rc = conv_grad_check(MM_F32, n, H, W, Cin, Cout, R, stride, pad, &Ho, &Wo);
  if (rc != MM_OK) return rc;
  *bytes = wgrad_nsplit((int64_t)n * Ho * Wo) * Cout * R * R * Cin * 4;
  return MM_OK;
}

extern "C" int mm_conv2d_nhwc_wgrad(int dtype, const void* dz, const void* x, int n, int H, int W, int Cin, int Cout, int R, int stride,
                                    int pad, void* dw, void* ws, int64_t ws_bytes, void* stream) {
  if (!dz || !x || !dw || !ws) return MM_ERR_ARG;
  int Ho = 0, Wo = 0;
  const int rc = conv_grad_check(dtype, n, H, W, Cin, Cout, R, stride, pad, &Ho, &Wo);
  if (rc != MM_OK) return rc;
  if ((Cin % 8) || (Cout % 64)) return MM_ERR_ALIGN;
  if (!mm_aligned16(dz) || !mm_aligned16(x) || !mm_aligned16(dw) || !mm_aligned16(ws)) return MM_ERR_ALIGN;
  const int64_t M = (int64_t)n * Ho * Wo, Mi = (int64_t)n * H * W, K = (int64_t)R * R * Cin;
  if (M > INT_MAX - 256 || Mi > INT_MAX - 256 || (int64_t)Cout * K > INT_MAX) return MM_ERR_UNSUPPORTED;
  const int64_t nsplit = wgrad_nsplit(M);
  if (nsplit > 65535) return MM_ERR_UNSUPPORTED;
  if (ws_bytes < nsplit * Cout * K * 4) return MM_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (M == 0) {
    if (hipMemsetAsync(dw, 0, (size_t)Cout * K * mm_elem_size(dtype), s) != hipSuccess) return MM_ERR_LAUNCH;
    return MM_OK;
  }
  ConvGradArgs a{dz, x, nullptr, nullptr, nullptr, (float*)ws, H, W, Cin, Ho, Wo, Cout, R, stride, pad, (int)M, (int)K, WG_SPLIT_ROWS};
  if (dtype == MM_BF16) {
    dim3 grid((unsigned)((K + 63) / 64), (unsigned)(Cout / 64), (unsigned)nsplit), block(256);
    hipLaunchKernelGGL(wgrad_bf16_kernel, grid, block, 0, s, a);
  } else {
    dim3 grid((unsigned)((Cout * K + 255) / 256), (unsigned)nsplit), block(256);
    hipLaunchKernelGGL(wgrad_f32_kernel, grid, block, 0, s, a);
  }
  MM_CHECK_LAUNCH();
  return mm_reduce_partials(dtype, (const float*)ws, (int)nsplit, (int)(Cout * K), dw, 0, stream);
}
