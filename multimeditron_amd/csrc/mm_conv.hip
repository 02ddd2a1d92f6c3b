// NHWC convolution kernels of the MoE gating network (a ResNet-50 in eval mode; model/modalities/gating.py).  The contract of
// the four entry points is written out in include/mm_hip.h; tests/conv_check.py restates it in fp64.
//
//   nchw_to_nhwc_kernel   fp32 pixels [n, C, H, W] -> [n, H, W, Cpad] in the storage type, channels C .. Cpad-1 zero
//   conv_bf16_kernel      implicit GEMM on v_mfma_f32_32x32x16_bf16, computed TRANSPOSED: D^T[cout, pixel] = W[cout, k] . X[k, pixel],
//                         k = (r * S + s) * Cin + c.  Cin % 8 == 0, so the 8 k-values one lane feeds to one MFMA are 8 contiguous
//                         channels of ONE filter tap: the weight fragment (A operand, lane = (cout & 31, k half)) and the
//                         activation fragment (B operand, lane = (pixel & 31, k half)) are each ONE 16-byte load straight into the
//                         operand registers -- no LDS, no barrier.  A tap outside the image (or a k-group past K, when
//                         K % 16 == 8) is a zero fragment and is never loaded.  One wave owns 64 couts x 32 pixels (two
//                         accumulators sharing the activation fragment), a workgroup 4 such waves along the pixels.  In the
//                         accumulator a lane holds ONE pixel and 4 x 4 consecutive couts per 32-cout tile, so the epilogue
//                         (acc * scale + shift (+ residual) (ReLU), all fp32, one rounding) loads scale / shift as 16-byte and the
//                         residual as 8-byte vectors and stores 8 bytes at a time.
//   conv_f32_kernel       the parity path: one thread per output element, four fmaf chains per filter tap summed tap by tap
//   maxpool_kernel        3x3 / stride 2 / pad 1, one thread per 16-byte channel vector of an output pixel
//   gate_head_kernel      one workgroup per image: fp32 mean over HW into LDS, one wave per expert logit, then softmax and top-k
#include "mm_common.h"

#include <limits.h>

namespace {

struct ConvArgs {
  const void* x;
  const void* w;
  const float* scale;
  const float* shift;
  const void* res;
  void* y;
  int H, W, Cin, Ho, Wo, Cout, S, stride, pad, relu;
  int M, K;   // M = n * Ho * Wo output pixels, K = R * S * Cin
};

template <typename T>
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ px, int64_t npix, int C, int64_t HW, int Cpad,
                                                           T* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // (image, h, w)
  if (i >= npix) return;
  const int64_t img = i / HW, hw = i - img * HW;
  const float* src = px + img * C * HW + hw;
  constexpr int N = Vec16<T>::N;
  Vec16<T>* dst = (Vec16<T>*)(out + i * Cpad);
  for (int c0 = 0; c0 < Cpad; c0 += N) {
    Vec16<T> v;
#pragma unroll
    for (int j = 0; j < N; ++j) v.set(j, c0 + j < C ? src[(int64_t)(c0 + j) * HW] : 0.f);
    dst[c0 / N] = v;
  }
}

__global__ __launch_bounds__(256) void conv_bf16_kernel(const ConvArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int m_wave = (blockIdx.x * 4 + wave) * 32;
  if (m_wave >= a.M) return;                                       // wave-uniform: the MFMAs below run with every lane on
  const int m = m_wave + r;                                        // this lane's output pixel
  const bool mv = m < a.M;
  const int co0 = blockIdx.y * 64;
  int hi0 = 0, wi0 = 0;
  const bf16* xb = (const bf16*)a.x;
  if (mv) {
    const int wo = m % a.Wo, t = m / a.Wo, ho = t % a.Ho, img = t / a.Ho;
    hi0 = ho * a.stride - a.pad;
    wi0 = wo * a.stride - a.pad;
    xb += (int64_t)img * a.H * a.W * a.Cin;
  }
  const bf16* w0 = (const bf16*)a.w + (int64_t)(co0 + r) * a.K;    // couts co0 + r and co0 + 32 + r
  const bf16* w1 = w0 + (int64_t)32 * a.K;
  const int cg = a.Cin >> 3, KG = a.K >> 3;                        // 8-channel groups per tap / in all
  int tap = h / cg, c8 = h - tap * cg;                             // this lane's k-group g = 2 * step + h as (rr, ss, c8)
  int rr = tap / a.S, ss = tap - rr * a.S;
  f32x16 acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int g = h; g - h < KG; g += 2) {
    bf16x8 fa0 = zero, fa1 = zero, fb = zero;
    if (g < KG) {
      fa0 = *(const bf16x8*)(w0 + g * 8);
      fa1 = *(const bf16x8*)(w1 + g * 8);
      const int hi = hi0 + rr, wi = wi0 + ss;
      if (mv && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W)
        fb = *(const bf16x8*)(xb + ((int64_t)hi * a.W + wi) * a.Cin + c8 * 8);
    }
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa0, fb, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa1, fb, acc1, 0, 0, 0);
    c8 += 2;
    while (c8 >= cg) {
      c8 -= cg;
      if (++ss == a.S) { ss = 0; ++rr; }
    }
  }
  if (!mv) return;
  // accumulator register i of a 32-cout tile: cout = (i & 3) + 8 * (i >> 2) + 4 * h, pixel = this lane's
  bf16* yrow = (bf16*)a.y + (int64_t)m * a.Cout;
  const bf16* rrow = a.res ? (const bf16*)a.res + (int64_t)m * a.Cout : nullptr;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int co = co0 + 32 * t + 8 * q + 4 * h;
      const f32x4 sc = *(const f32x4*)(a.scale + co), sh = *(const f32x4*)(a.shift + co);
      bf16x4 rv = {0, 0, 0, 0};
      if (rrow) rv = *(const bf16x4*)(rrow + co);
      bf16x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v = __builtin_fmaf(t ? acc1[4 * q + j] : acc0[4 * q + j], sc[j], sh[j]);
        if (rrow) v += (float)rv[j];
        if (a.relu) v = fmaxf(v, 0.f);
        o[j] = (bf16)v;
      }
      *(bf16x4*)(yrow + co) = o;
    }
  }
}

__global__ __launch_bounds__(256) void conv_f32_kernel(const ConvArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)a.M * a.Cout) return;
  const int co = (int)(idx % a.Cout), m = (int)(idx / a.Cout);
  const int wo = m % a.Wo, t = m / a.Wo, ho = t % a.Ho, img = t / a.Ho;
  const int hi0 = ho * a.stride - a.pad, wi0 = wo * a.stride - a.pad;
  const float* xb = (const float*)a.x + (int64_t)img * a.H * a.W * a.Cin;
  const float* wb = (const float*)a.w + (int64_t)co * a.K;
  const int R = a.K / (a.S * a.Cin);
  float acc = 0.f;
  for (int rr = 0; rr < R; ++rr) {
    const int hi = hi0 + rr;
    if ((unsigned)hi >= (unsigned)a.H) continue;
    for (int ss = 0; ss < a.S; ++ss) {
      const int wi = wi0 + ss;
      if ((unsigned)wi >= (unsigned)a.W) continue;
      const f32x4* xp = (const f32x4*)(xb + ((int64_t)hi * a.W + wi) * a.Cin);
      const f32x4* wp = (const f32x4*)(wb + (int64_t)(rr * a.S + ss) * a.Cin);
      f32x4 part = {0.f, 0.f, 0.f, 0.f};                           // four chains per tap, summed per tap: short fp32 chains
      for (int c = 0; c < a.Cin / 4; ++c) {
        const f32x4 xv = xp[c], wv = wp[c];
#pragma unroll
        for (int j = 0; j < 4; ++j) part[j] = __builtin_fmaf(xv[j], wv[j], part[j]);
      }
      acc += (part[0] + part[1]) + (part[2] + part[3]);
    }
  }
  float v = __builtin_fmaf(acc, a.scale[co], a.shift[co]);
  if (a.res) v += ((const float*)a.res)[idx];
  if (a.relu) v = fmaxf(v, 0.f);
  ((float*)a.y)[idx] = v;
}

template <typename T>
__global__ __launch_bounds__(256) void maxpool_kernel(const T* __restrict__ x, int H, int W, int C, int Ho, int Wo, int64_t total,
                                                      T* __restrict__ y) {
  constexpr int N = Vec16<T>::N;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // (image, ho, wo, channel vector)
  if (i >= total) return;
  const int cv = C / N;
  const int v = (int)(i % cv);
  int64_t t = i / cv;
  const int wo = (int)(t % Wo);
  t /= Wo;
  const int ho = (int)(t % Ho);
  const int64_t img = t / Ho;
  float best[N];
#pragma unroll
  for (int j = 0; j < N; ++j) best[j] = -INFINITY;
#pragma unroll
  for (int dr = 0; dr < 3; ++dr) {
    const int hi = 2 * ho - 1 + dr;
    if ((unsigned)hi >= (unsigned)H) continue;                     // padding taps take no part in the maximum
#pragma unroll
    for (int ds = 0; ds < 3; ++ds) {
      const int wi = 2 * wo - 1 + ds;
      if ((unsigned)wi >= (unsigned)W) continue;
      const Vec16<T> xv = *(const Vec16<T>*)(x + ((img * H + hi) * W + wi) * C + (int64_t)v * N);
#pragma unroll
      for (int j = 0; j < N; ++j) best[j] = fmaxf(best[j], xv.get(j));
    }
  }
  Vec16<T> o;
#pragma unroll
  for (int j = 0; j < N; ++j) o.set(j, best[j]);
  *(Vec16<T>*)(y + i * N) = o;
}

constexpr int GATE_MAX_C = 8192;       // pooled row in LDS (32 KiB)
constexpr int GATE_MAX_E = 64;

template <typename T>
__global__ __launch_bounds__(256) void gate_head_kernel(const T* __restrict__ x, int HW, int C, const T* __restrict__ fc_w,
                                                        const T* __restrict__ fc_b, int E, int top_k, T* __restrict__ logits,
                                                        T* __restrict__ weights, int64_t* __restrict__ topk) {
  __shared__ float pooled[GATE_MAX_C];
  __shared__ float lg[GATE_MAX_E];
  constexpr int N = Vec16<T>::N;
  const int img = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T* xi = x + (int64_t)img * HW * C;
  const float inv = 1.f / (float)HW;
  for (int v = threadIdx.x; v < C / N; v += 256) {                 // fp32 sum over HW in order, then one multiply by 1 / HW
    float s[N];
#pragma unroll
    for (int j = 0; j < N; ++j) s[j] = 0.f;
    for (int p = 0; p < HW; ++p) {
      const Vec16<T> xv = *(const Vec16<T>*)(xi + (int64_t)p * C + v * N);
#pragma unroll
      for (int j = 0; j < N; ++j) s[j] += xv.get(j);
    }
#pragma unroll
    for (int j = 0; j < N; ++j) pooled[v * N + j] = s[j] * inv;
  }
  __syncthreads();
  for (int e = wave; e < E; e += 4) {                              // one wave per logit
    const T* wr = fc_w + (int64_t)e * C;
    float d = 0.f;
    for (int v = lane; v < C / N; v += 64) {
      const Vec16<T> wv = *(const Vec16<T>*)(wr + v * N);
#pragma unroll
      for (int j = 0; j < N; ++j) d = __builtin_fmaf(pooled[v * N + j], wv.get(j), d);
    }
    d = wave_sum(d);
    if (lane == 0) {
      const T l = from_f32<T>(d + to_f32(fc_b[e]));                // the logit in the storage type: softmax and top-k read THIS value
      logits[(int64_t)img * E + e] = l;
      lg[e] = to_f32(l);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float mx = -INFINITY;
    for (int e = 0; e < E; ++e) mx = fmaxf(mx, lg[e]);
    float sum = 0.f;
    for (int e = 0; e < E; ++e) sum += expf(lg[e] - mx);
    for (int e = 0; e < E; ++e) weights[(int64_t)img * E + e] = from_f32<T>(expf(lg[e] - mx) / sum);
    unsigned long long used = 0ull;                                // top_k largest logits, descending, lower index first on ties
    for (int k = 0; k < top_k; ++k) {
      int best = -1;
      for (int e = 0; e < E; ++e)
        if (!((used >> e) & 1ull) && (best < 0 || lg[e] > lg[best])) best = e;
      used |= 1ull << best;
      topk[(int64_t)img * top_k + k] = best;
    }
  }
}

}  // namespace

extern "C" int mm_nchw_to_nhwc(int dtype, const float* pixels, int n, int C, int H, int W, int Cpad, void* out, void* stream) {
  if (!pixels || !out || n < 0 || C <= 0 || H <= 0 || W <= 0 || Cpad < C) return MM_ERR_ARG;
  if (dtype != MM_BF16 && dtype != MM_F32) return MM_ERR_UNSUPPORTED;
  if ((Cpad % (dtype == MM_BF16 ? 8 : 4)) || !mm_aligned16(out)) return MM_ERR_ALIGN;
  const int64_t npix = (int64_t)n * H * W;
  if (npix == 0) return MM_OK;
  if ((npix + 255) / 256 > INT_MAX) return MM_ERR_UNSUPPORTED;
  dim3 grid((unsigned)((npix + 255) / 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MM_BF16)
    hipLaunchKernelGGL(nchw_to_nhwc_kernel<bf16>, grid, block, 0, s, pixels, npix, C, (int64_t)H * W, Cpad, (bf16*)out);
  else
    hipLaunchKernelGGL(nchw_to_nhwc_kernel<float>, grid, block, 0, s, pixels, npix, C, (int64_t)H * W, Cpad, (float*)out);
  MM_CHECK_LAUNCH();
  return MM_OK;
}

extern "C" int mm_conv2d_nhwc_fwd(int dtype, const void* x, int n, int H, int W, int Cin, const void* w, int Cout, int R, int stride,
                                  int pad, const float* scale, const float* shift, const void* residual, int relu, void* y,
                                  void* stream) {
  if (!x || !w || !scale || !shift || !y || n < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || pad < 0) return MM_ERR_ARG;
  if (dtype != MM_BF16 && dtype != MM_F32) return MM_ERR_UNSUPPORTED;
  if ((R != 1 && R != 3 && R != 7) || (stride != 1 && stride != 2) || (pad != 0 && pad != 1 && pad != 3)) return MM_ERR_UNSUPPORTED;
  if ((Cin % 8) || (Cout % 64)) return MM_ERR_ALIGN;
  if (!mm_aligned16(x) || !mm_aligned16(w) || !mm_aligned16(scale) || !mm_aligned16(shift) || !mm_aligned16(y) ||
      (residual && !mm_aligned16(residual)))
    return MM_ERR_ALIGN;
  if (H + 2 * pad < R || W + 2 * pad < R) return MM_ERR_ARG;
  const int Ho = (H + 2 * pad - R) / stride + 1, Wo = (W + 2 * pad - R) / stride + 1;
  const int64_t M = (int64_t)n * Ho * Wo, K = (int64_t)R * R * Cin;
  if (M > INT_MAX - 256 || (int64_t)Cout * K > INT_MAX || M * Cout / 256 > INT_MAX - 1) return MM_ERR_UNSUPPORTED;
  if (M == 0) return MM_OK;
  ConvArgs a{x, w, scale, shift, residual, y, H, W, Cin, Ho, Wo, Cout, R, stride, pad, relu ? 1 : 0, (int)M, (int)K};
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MM_BF16) {
    dim3 grid((unsigned)((M + 127) / 128), (unsigned)(Cout / 64)), block(256);
    hipLaunchKernelGGL(conv_bf16_kernel, grid, block, 0, s, a);
  } else {
    dim3 grid((unsigned)((M * Cout + 255) / 256)), block(256);
    hipLaunchKernelGGL(conv_f32_kernel, grid, block, 0, s, a);
  }
  MM_CHECK_LAUNCH();
  return MM_OK;
}

extern "C" int mm_maxpool2d_nhwc(int dtype, const void* x, int n, int H, int W, int C, void* y, void* stream) {
  if (!x || !y || n < 0 || H <= 0 || W <= 0 || C <= 0) return MM_ERR_ARG;
  if (dtype != MM_BF16 && dtype != MM_F32) return MM_ERR_UNSUPPORTED;
  const int vn = dtype == MM_BF16 ? 8 : 4;
  if ((C % vn) || !mm_aligned16(x) || !mm_aligned16(y)) return MM_ERR_ALIGN;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const int64_t total = (int64_t)n * Ho * Wo * (C / vn);
  if (total == 0) return MM_OK;
  if ((total + 255) / 256 > INT_MAX) return MM_ERR_UNSUPPORTED;
  dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MM_BF16)
    hipLaunchKernelGGL(maxpool_kernel<bf16>, grid, block, 0, s, (const bf16*)x, H, W, C, Ho, Wo, total, (bf16*)y);
  else
    hipLaunchKernelGGL(maxpool_kernel<float>, grid, block, 0, s, (const float*)x, H, W, C, Ho, Wo, total, (float*)y);
  MM_CHECK_LAUNCH();
  return MM_OK;
}

extern "C" int mm_gate_head(int dtype, const void* x, int n, int HW, int C, const void* fc_w, const void* fc_b, int E, int top_k,
                            void* logits, void* weights, int64_t* topk_idx, void* stream) {
  if (!x || !fc_w || !fc_b || !logits || !weights || !topk_idx || n < 0 || HW <= 0 || C <= 0 || E <= 0) return MM_ERR_ARG;
  if (top_k < 1 || top_k > E) return MM_ERR_ARG;
  if (dtype != MM_BF16 && dtype != MM_F32) return MM_ERR_UNSUPPORTED;
  if (E > GATE_MAX_E || C > GATE_MAX_C) return MM_ERR_UNSUPPORTED;
  if ((C % (dtype == MM_BF16 ? 8 : 4)) || !mm_aligned16(x) || !mm_aligned16(fc_w)) return MM_ERR_ALIGN;
  if (n == 0) return MM_OK;
  dim3 grid((unsigned)n), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MM_BF16)
    hipLaunchKernelGGL(gate_head_kernel<bf16>, grid, block, 0, s, (const bf16*)x, HW, C, (const bf16*)fc_w, (const bf16*)fc_b, E, top_k,
                       (bf16*)logits, (bf16*)weights, topk_idx);
  else
    hipLaunchKernelGGL(gate_head_kernel<float>, grid, block, 0, s, (const float*)x, HW, C, (const float*)fc_w, (const float*)fc_b, E,
                       top_k, (float*)logits, (float*)weights, topk_idx);
  MM_CHECK_LAUNCH();
  return MM_OK;
}
