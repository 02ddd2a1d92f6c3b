// xIELU, the activation of the Apertus MLP `down_proj(xIELU(up_proj(x)))` (HF 5.15 models/apertus/modeling_apertus.py ApertusMLP,
// activations.py XIELUActivation._xielu_python), forward and backward, plus the finishing sum of the two scalar gradients.
//   ap = softplus(alpha_p_raw), an = beta + softplus(alpha_n_raw)
//   y  = x > 0 ? ap x^2 + beta x : an (expm1(min(x, eps)) - x) + beta x
// HBM-bound streaming kernels: 16-byte loads and stores, a workgroup of 256 lanes owns a contiguous run of iters * 2048 elements
// (iters a function of n alone), the one lane whose vector straddles n finishes it element by element.  All arithmetic fp32, one
// rounding per output.  The scalar gradients: every lane sums its terms in element order, wave64 shuffles and 4 LDS words give the
// workgroup's two sums (partials[2b], partials[2b+1]), mm_xielu_reduce adds the workgroups in a fixed order: no atomics, same bits on
// every launch.
#include "mm_common.h"

namespace {

constexpr int XIELU_WG_ELEMS = 2048;       // elements of one workgroup per pass: 1 vector per lane (bf16), 2 (f32)
constexpr int XIELU_MAX_BLOCKS = 4096;     // past 2048 * 4096 elements a workgroup takes several passes

// torch softplus (beta 1, threshold 20) and its derivative
__device__ __forceinline__ float softplus20(float a) { return a > 20.f ? a : log1pf(expf(a)); }
__device__ __forceinline__ float softplus20_grad(float a) { return a > 20.f ? 1.f : 1.f / (1.f + expf(-a)); }

// expm1(x) for x <= 0 in ~12 VALU operations (the library's expm1f would make the kernels VALU-bound at Apertus-8B width):
// -0.35 < x: x + x^2 (1/2 + x/6 + ... + x^5/5040) in Horner form (truncation x^8/40320: 1.6e-8 relative); otherwise
// exp(x) - 1 with the hardware exp2 (|exp(x) - 1| >= 0.29 there, so the absolute error of exp, <= ~1e-7 * |x| exp(x), stays ~1 ulp).
__device__ __forceinline__ float expm1_neg(float x) {
  float q = 1.f / 5040.f;
  q = __builtin_fmaf(q, x, 1.f / 720.f);
  q = __builtin_fmaf(q, x, 1.f / 120.f);
  q = __builtin_fmaf(q, x, 1.f / 24.f);
  q = __builtin_fmaf(q, x, 1.f / 6.f);
  q = __builtin_fmaf(q, x, 0.5f);
  const float small = __builtin_fmaf(x * x, q, x);
  const float big = __expf(x) - 1.f;
  return x > -0.35f ? small : big;
}

struct XieluParams { float ap, an, beta, eps; };

template <typename T>
__device__ __forceinline__ XieluParams xielu_params(const T* ap_raw, const T* an_raw, float beta, float eps) {
  XieluParams p;
  p.ap = softplus20(to_f32(*ap_raw));
  p.an = beta + softplus20(to_f32(*an_raw));
  p.beta = beta;
  p.eps = eps;
  return p;
}

__device__ __forceinline__ float xielu_y(float x, const XieluParams& p) {
  const float pos = __builtin_fmaf(p.ap, x, p.beta) * x;
  const float neg = __builtin_fmaf(p.an, expm1_neg(fminf(x, p.eps)) - x, p.beta * x);
  return x > 0.f ? pos : neg;
}

// dx = dy * y'(x); tp / tn: this element's terms of the two scalar sums (one of them is 0)
__device__ __forceinline__ float xielu_dx(float x, float dy, const XieluParams& p, float& tp, float& tn) {
  const float em = expm1_neg(fminf(x, p.eps));
  // torch.min splits the gradient at a tie: 1 below eps, 1/2 at eps, 0 above (exp(eps) = em + 1 there)
  const float ge = x < p.eps ? em : (x == p.eps ? __builtin_fmaf(0.5f, em, -0.5f) : -1.f);
  const bool pos = x > 0.f;
  const float g = pos ? __builtin_fmaf(p.ap + p.ap, x, p.beta) : __builtin_fmaf(p.an, ge, p.beta);
  tp = pos ? dy * x * x : 0.f;
  tn = pos ? 0.f : dy * (em - x);
  return dy * g;
}

template <typename T>
__global__ __launch_bounds__(256) void xielu_fwd_kernel(const T* x, int64_t n, int iters, const T* ap_raw, const T* an_raw, float beta,
                                                       float eps, T* y) {
  constexpr int VN = Vec16<T>::N, VPL = XIELU_WG_ELEMS / 256 / VN;
  const XieluParams p = xielu_params<T>(ap_raw, an_raw, beta, eps);
  const int64_t base = (int64_t)blockIdx.x * iters * XIELU_WG_ELEMS;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      const int64_t i = base + (int64_t)it * XIELU_WG_ELEMS + (v * 256 + (int)threadIdx.x) * VN;
      if (i + VN <= n) {
        const Vec16<T> a = *(const Vec16<T>*)(x + i);
        Vec16<T> o;
#pragma unroll
        for (int k = 0; k < VN; ++k) o.set(k, xielu_y(a.get(k), p));
        *(Vec16<T>*)(y + i) = o;
      } else {
        for (int64_t j = i; j < n; ++j) y[j] = from_f32<T>(xielu_y(to_f32(x[j]), p));      // the tail: fewer than VN elements, one lane
      }
    }
  }
}

template <typename T, bool SUMS>
__global__ __launch_bounds__(256) void xielu_bwd_kernel(const T* x, const T* dy, int64_t n, int iters, const T* ap_raw, const T* an_raw,
                                                       float beta, float eps, T* dx, float* partials) {
  constexpr int VN = Vec16<T>::N, VPL = XIELU_WG_ELEMS / 256 / VN;
  __shared__ float red[8];
  const XieluParams p = xielu_params<T>(ap_raw, an_raw, beta, eps);
  const int64_t base = (int64_t)blockIdx.x * iters * XIELU_WG_ELEMS;
  float sp = 0.f, sn = 0.f;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      const int64_t i = base + (int64_t)it * XIELU_WG_ELEMS + (v * 256 + (int)threadIdx.x) * VN;
      if (i + VN <= n) {
        const Vec16<T> a = *(const Vec16<T>*)(x + i), d = *(const Vec16<T>*)(dy + i);
        Vec16<T> o;
#pragma unroll
        for (int k = 0; k < VN; ++k) {
          float tp, tn;
          o.set(k, xielu_dx(a.get(k), d.get(k), p, tp, tn));
          sp += tp;
          sn += tn;
        }
        *(Vec16<T>*)(dx + i) = o;
      } else {
        for (int64_t j = i; j < n; ++j) {
          float tp, tn;
          dx[j] = from_f32<T>(xielu_dx(to_f32(x[j]), to_f32(dy[j]), p, tp, tn));
          sp += tp;
          sn += tn;
        }
      }
    }
  }
  if (SUMS) {
    sp = block_sum_256(sp, red);
    sn = block_sum_256(sn, red);
    if (threadIdx.x == 0) {
      partials[2 * (int64_t)blockIdx.x] = sp;
      partials[2 * (int64_t)blockIdx.x + 1] = sn;
    }
  }
}

// dalpha_p_raw (+)= sp'(alpha_p_raw) * sum_b partials[2b], dalpha_n_raw likewise from partials[2b+1]: ONE workgroup; lane l adds
// workgroups l, l + 256, ... in that order, then block_sum_256's fixed tree (reduce_partials_kernel's scheme for two columns).
template <typename T>
__global__ __launch_bounds__(256) void xielu_reduce_kernel(const float* partials, int nblk, const T* ap_raw, const T* an_raw, T* dap, T* dan,
                                                          int acc_p, int acc_n) {
  __shared__ float red[8];
  float sp = 0.f, sn = 0.f;
  for (int b = threadIdx.x; b < nblk; b += 256) {
    const f32x2 v = *(const f32x2*)(partials + 2 * (int64_t)b);
    sp += v[0];
    sn += v[1];
  }
  sp = block_sum_256(sp, red);
  sn = block_sum_256(sn, red);
  if (threadIdx.x == 0) {
    float gp = softplus20_grad(to_f32(*ap_raw)) * sp, gn = softplus20_grad(to_f32(*an_raw)) * sn;
    if (acc_p) gp += to_f32(*dap);
    if (acc_n) gn += to_f32(*dan);
    *dap = from_f32<T>(gp);
    *dan = from_f32<T>(gn);
  }
}

inline int xielu_iters(int64_t n) {
  const int64_t runs = (n + XIELU_WG_ELEMS - 1) / XIELU_WG_ELEMS;
  const int64_t it = (runs + XIELU_MAX_BLOCKS - 1) / XIELU_MAX_BLOCKS;
  return it < 1 ? 1 : (int)it;
}

}  // namespace

extern "C" int mm_xielu_bwd_blocks(int64_t n) {
  if (n <= 0) return 0;
  const int64_t chunk = (int64_t)xielu_iters(n) * XIELU_WG_ELEMS;
  return (int)((n + chunk - 1) / chunk);
}

extern "C" int mm_xielu_fwd(int dtype, const void* x, int64_t n, const void* alpha_p_raw, const void* alpha_n_raw, float beta, float eps,
                            void* y, void* stream) {
  if (!x || !y || !alpha_p_raw || !alpha_n_raw || n < 0) return MM_ERR_ARG;
  if (dtype != MM_BF16 && dtype != MM_F32) return MM_ERR_UNSUPPORTED;
  if (!mm_aligned16(x) || !mm_aligned16(y)) return MM_ERR_ALIGN;
  if (n == 0) return MM_OK;
  dim3 grid((unsigned)mm_xielu_bwd_blocks(n)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MM_BF16)
    hipLaunchKernelGGL(xielu_fwd_kernel<bf16>, grid, block, 0, s, (const bf16*)x, n, xielu_iters(n), (const bf16*)alpha_p_raw,
                       (const bf16*)alpha_n_raw, beta, eps, (bf16*)y);
  else
    hipLaunchKernelGGL(xielu_fwd_kernel<float>, grid, block, 0, s, (const float*)x, n, xielu_iters(n), (const float*)alpha_p_raw,
                       (const float*)alpha_n_raw, beta, eps, (float*)y);
  MM_CHECK_LAUNCH();
  return MM_OK;
}

extern "C" int mm_xielu_bwd(int dtype, const void* x, const void* dy, int64_t n, const void* alpha_p_raw, const void* alpha_n_raw, float beta,
                            float eps, void* dx, float* partials, void* stream) {
  if (!x || !dy || !dx || !alpha_p_raw || !alpha_n_raw || n < 0) return MM_ERR_ARG;
  if (dtype != MM_BF16 && dtype != MM_F32) return MM_ERR_UNSUPPORTED;
  if (!mm_aligned16(x) || !mm_aligned16(dy) || !mm_aligned16(dx) || (((uintptr_t)partials) & 7)) return MM_ERR_ALIGN;
  if (n == 0) return MM_OK;
  dim3 grid((unsigned)mm_xielu_bwd_blocks(n)), block(256);
  hipStream_t s = (hipStream_t)stream;
  const int iters = xielu_iters(n);
#define XIELU_BWD(T, SUMS)                                                                                                         \
  hipLaunchKernelGGL((xielu_bwd_kernel<T, SUMS>), grid, block, 0, s, (const T*)x, (const T*)dy, n, iters, (const T*)alpha_p_raw, \
                     (const T*)alpha_n_raw, beta, eps, (T*)dx, partials)
  if (dtype == MM_BF16) {
    if (partials) XIELU_BWD(bf16, true); else XIELU_BWD(bf16, false);
  } else {
    if (partials) XIELU_BWD(float, true); else XIELU_BWD(float, false);
  }
#undef XIELU_BWD
  MM_CHECK_LAUNCH();
  return MM_OK;
}

extern "C" int mm_xielu_reduce(int dtype, const float* partials, int nblk, const void* alpha_p_raw, const void* alpha_n_raw,
                               void* dalpha_p_raw, void* dalpha_n_raw, int accumulate_p, int accumulate_n, void* stream) {
  if (!partials || !alpha_p_raw || !alpha_n_raw || !dalpha_p_raw || !dalpha_n_raw || nblk < 0) return MM_ERR_ARG;
  if (dtype != MM_BF16 && dtype != MM_F32) return MM_ERR_UNSUPPORTED;
  if (((uintptr_t)partials) & 7) return MM_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MM_BF16)
    hipLaunchKernelGGL(xielu_reduce_kernel<bf16>, dim3(1), dim3(256), 0, s, partials, nblk, (const bf16*)alpha_p_raw, (const bf16*)alpha_n_raw,
                       (bf16*)dalpha_p_raw, (bf16*)dalpha_n_raw, accumulate_p, accumulate_n);
  else
    hipLaunchKernelGGL(xielu_reduce_kernel<float>, dim3(1), dim3(256), 0, s, partials, nblk, (const float*)alpha_p_raw,
                       (const float*)alpha_n_raw, (float*)dalpha_p_raw, (float*)dalpha_n_raw, accumulate_p, accumulate_n);
  MM_CHECK_LAUNCH();
  return MM_OK;
}
