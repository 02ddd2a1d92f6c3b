// Qwen3's per-head q/k RMSNorm fused with RoPE (HF 5.15 models/qwen3/modeling_qwen3.py:50-64,237-257):
//   q = RoPE(q_norm(q_proj(h).view(.., Hq, D)));  k = RoPE(k_norm(k_proj(h).view(.., Hkv, D)))
// One pass over the q|k heads of the fused projection output for forward, backward and the decode step.
// Lane mapping (rope_apply_kernel's): a lane owns VN consecutive j of one (token, head) and the VN elements at j + D/2, so
// the rotation needs no lane exchange; a head is LPH = D/2/VN consecutive lanes (8 for bf16 D=128) and its sum of squares
// is a log2(LPH)-step xor-shuffle inside them: no LDS, no barrier in forward.  16-byte loads and stores throughout.
#include "mm_common.h"

namespace {

constexpr int QKN_BWD_ROWS_PER_BLOCK = 8;     // T = 8192 -> 1024 workgroups; dw partials [nblk, D] f32

// rstd of one head: fp32 sum of squares over the LPH lanes that hold it, then rmsnorm_fwd_kernel's rsqrtf(ss/D + eps).
// Shared by the forward and the decode-append kernels so that the two agree bit for bit.
template <typename T, int D>
__device__ __forceinline__ float head_rstd(const Vec16<T>& a, const Vec16<T>& b, float eps) {
  constexpr int LPH = D / 2 / Vec16<T>::N;
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < Vec16<T>::N; ++k) {
    const float fa = a.get(k), fb = b.get(k);
    ss += fa * fa;
    ss += fb * fb;
  }
#pragma unroll
  for (int o = LPH / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  return rsqrtf(ss / (float)D + eps);
}

// y = bf16(w * bf16(x * rs)) (rmsnorm_fwd_kernel's rounding points), then rope_apply_kernel's rotation of the rounded y
template <typename T>
__device__ __forceinline__ void norm_rope(const Vec16<T>& a, const Vec16<T>& b, const Vec16<T>& wa, const Vec16<T>& wb, float rs,
                                          const float* c, const float* s, Vec16<T>& oa, Vec16<T>& ob) {
#pragma unroll
  for (int k = 0; k < Vec16<T>::N; ++k) {
    const float ya = to_f32(from_f32<T>(wa.get(k) * to_f32(from_f32<T>(a.get(k) * rs))));
    const float yb = to_f32(from_f32<T>(wb.get(k) * to_f32(from_f32<T>(b.get(k) * rs))));
    oa.set(k, rope_lo(ya, yb, c[k], s[k]));
    ob.set(k, rope_hi(ya, yb, c[k], s[k]));
  }
}

// x viewed [T, Hq+Hkv, D] (row stride ld_in) -> y [T, Hq+Hkv, D] (row stride ld_out), rstd [T, Hq+Hkv].  y may equal x
// (same stride): every lane stores only the elements it loaded.
template <typename T, int D>
__global__ __launch_bounds__(256) void qk_norm_rope_fwd_kernel(const T* x, int ld_in, int Tn, int Hq, int Hkv, const T* wq, const T* wk,
                                                              float eps, const float* cs, const float* sn, T* y, int ld_out, float* rstd) {
  constexpr int VN = Vec16<T>::N, HALF = D / 2, LPH = HALF / VN;
  const int nh = Hq + Hkv;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)Tn * nh * LPH) return;          // a head's lanes are all in or all out (256 % LPH == 0)
  const int jc = (int)(i % LPH);
  const int64_t hh = i / LPH;                        // t * nh + h
  const int h = (int)(hh % nh), t = (int)(hh / nh);
  const T* p = x + (int64_t)t * ld_in + h * D + jc * VN;
  const Vec16<T> a = *(const Vec16<T>*)p, b = *(const Vec16<T>*)(p + HALF);
  const T* w = (h < Hq ? wq : wk) + jc * VN;
  const Vec16<T> wa = *(const Vec16<T>*)w, wb = *(const Vec16<T>*)(w + HALF);
  const float rs = head_rstd<T, D>(a, b, eps);
  Vec16<T> oa, ob;
  norm_rope<T>(a, b, wa, wb, rs, cs + (int64_t)t * HALF + jc * VN, sn + (int64_t)t * HALF + jc * VN, oa, ob);
  T* q = y + (int64_t)t * ld_out + h * D + jc * VN;
  *(Vec16<T>*)q = oa;
  *(Vec16<T>*)(q + HALF) = ob;
  if (rstd && jc == 0) rstd[hh] = rs;
}

// decode step: the forward above in place on the q|k heads of x [T, (Hq+2Hkv)*D] (row stride ld) plus the append of the normed,
// roped k heads and of the v heads to the KV cache row (rope_append_kernel's layout)
template <typename T, int D>
__global__ __launch_bounds__(256) void qk_norm_rope_append_kernel(T* x, int ld, int Tn, int Hq, int Hkv, const T* wq, const T* wk,
                                                                 float eps, const float* cs, const float* sn, T* kdst, T* vdst,
                                                                 int64_t dstride) {
  constexpr int VN = Vec16<T>::N, HALF = D / 2, LPH = HALF / VN;
  const int nh = Hq + 2 * Hkv;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)Tn * nh * LPH) return;
  const int jc = (int)(i % LPH);
  const int h = (int)((i / LPH) % nh), t = (int)(i / ((int64_t)LPH * nh));
  T* p = x + (int64_t)t * ld + h * D + jc * VN;
  Vec16<T> a = *(Vec16<T>*)p, b = *(Vec16<T>*)(p + HALF), oa = a, ob = b;
  if (h < Hq + Hkv) {                                // uniform over the head's lanes
    const T* w = (h < Hq ? wq : wk) + jc * VN;
    const Vec16<T> wa = *(const Vec16<T>*)w, wb = *(const Vec16<T>*)(w + HALF);
    const float rs = head_rstd<T, D>(a, b, eps);
    norm_rope<T>(a, b, wa, wb, rs, cs + (int64_t)t * HALF + jc * VN, sn + (int64_t)t * HALF + jc * VN, oa, ob);
    *(Vec16<T>*)p = oa;
    *(Vec16<T>*)(p + HALF) = ob;
  }
  if (h >= Hq) {
    T* d = (h < Hq + Hkv ? kdst + (h - Hq) * D : vdst + (h - Hq - Hkv) * D) + (int64_t)t * dstride + jc * VN;
    *(Vec16<T>*)d = oa;
    *(Vec16<T>*)(d + HALF) = ob;
  }
}

// backward: g = inverse RoPE of dqk (kept in fp32), then rmsnorm_bwd_kernel's dx = rs*(g*w - xh*mean(g*w*xh)), xh = x*rs, into the
// q|k columns of dx; dw partial of a block = sum over its rows of g*xh, per head kind (q / k).  A block owns QKN_BWD_ROWS_PER_BLOCK
// tokens; a lane keeps its columns (jc fixed, 256 % LPH == 0) for the whole loop and its partial sums in registers, then the
// NS = 256/LPH lanes of each column are summed through LDS in a fixed order: deterministic, no atomics.
template <typename T, int D>
__global__ __launch_bounds__(256) void qk_norm_rope_bwd_kernel(const T* dqk, int ld_dqk, const T* x, int ld_x, int Tn, int Hq, int Hkv,
                                                              const T* wq, const T* wk, const float* rstd, const float* cs,
                                                              const float* sn, T* dx, int ld_dx, float* dwq, float* dwk) {
  constexpr int VN = Vec16<T>::N, HALF = D / 2, LPH = HALF / VN, NS = 256 / LPH;
  __shared__ float red[2][NS][D];                    // 32 KB (bf16) / 16 KB (f32)
  const int nh = Hq + Hkv, jc = threadIdx.x % LPH;
  const Vec16<T> wqa = *(const Vec16<T>*)(wq + jc * VN), wqb = *(const Vec16<T>*)(wq + HALF + jc * VN);
  const Vec16<T> wka = *(const Vec16<T>*)(wk + jc * VN), wkb = *(const Vec16<T>*)(wk + HALF + jc * VN);
  float aq[2 * VN], ak[2 * VN];
#pragma unroll
  for (int k = 0; k < 2 * VN; ++k) { aq[k] = 0.f; ak[k] = 0.f; }
  const int r0 = blockIdx.x * QKN_BWD_ROWS_PER_BLOCK;
  const int r1 = min(Tn, r0 + QKN_BWD_ROWS_PER_BLOCK);
  const int items = (r1 - r0) * nh * LPH;
  for (int it = threadIdx.x; it < items; it += 256) {
    const int hh = it / LPH, h = hh % nh, t = r0 + hh / nh;
    const bool isq = h < Hq;
    const T* pg = dqk + (int64_t)t * ld_dqk + h * D + jc * VN;
    const T* px = x + (int64_t)t * ld_x + h * D + jc * VN;
    const Vec16<T> ga = *(const Vec16<T>*)pg, gb = *(const Vec16<T>*)(pg + HALF);
    const Vec16<T> xa = *(const Vec16<T>*)px, xb = *(const Vec16<T>*)(px + HALF);
    const float rs = rstd[(int64_t)t * nh + h];
    const float* c = cs + (int64_t)t * HALF + jc * VN;
    const float* s = sn + (int64_t)t * HALF + jc * VN;
    float gya[VN], gyb[VN], dot = 0.f;
#pragma unroll
    for (int k = 0; k < VN; ++k) {
      gya[k] = rope_lo(ga.get(k), gb.get(k), c[k], -s[k]);      // adjoint rotation
      gyb[k] = rope_hi(ga.get(k), gb.get(k), c[k], -s[k]);
      const float wa = isq ? wqa.get(k) : wka.get(k), wb = isq ? wqb.get(k) : wkb.get(k);
      const float xha = xa.get(k) * rs, xhb = xb.get(k) * rs;
      dot += gya[k] * wa * xha;
      dot += gyb[k] * wb * xhb;
      const float da = gya[k] * xha, db = gyb[k] * xhb;
      aq[k] += isq ? da : 0.f;
      aq[VN + k] += isq ? db : 0.f;
      ak[k] += isq ? 0.f : da;
      ak[VN + k] += isq ? 0.f : db;
    }
#pragma unroll
    for (int o = LPH / 2; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
    dot /= (float)D;
    Vec16<T> oa, ob;
#pragma unroll
    for (int k = 0; k < VN; ++k) {
      const float wa = isq ? wqa.get(k) : wka.get(k), wb = isq ? wqb.get(k) : wkb.get(k);
      oa.set(k, rs * (gya[k] * wa - xa.get(k) * rs * dot));
      ob.set(k, rs * (gyb[k] * wb - xb.get(k) * rs * dot));
    }
    T* q = dx + (int64_t)t * ld_dx + h * D + jc * VN;
    *(Vec16<T>*)q = oa;
    *(Vec16<T>*)(q + HALF) = ob;
  }
  if (!dwq) return;                                  // frozen norms: dx only (uniform over the grid)
  const int slot = threadIdx.x / LPH;
#pragma unroll
  for (int k = 0; k < VN; ++k) {
    red[0][slot][jc * VN + k] = aq[k];
    red[0][slot][HALF + jc * VN + k] = aq[VN + k];
    red[1][slot][jc * VN + k] = ak[k];
    red[1][slot][HALF + jc * VN + k] = ak[VN + k];
  }
  __syncthreads();
  for (int o = threadIdx.x; o < 2 * D; o += 256) {
    const int which = o / D, col = o % D;
    float sum = 0.f;
#pragma unroll 8
    for (int sl = 0; sl < NS; ++sl) sum += red[which][sl][col];
    (which ? dwk : dwq)[(int64_t)blockIdx.x * D + col] = sum;
  }
}

}  // namespace

#define QKN_DISPATCH(D, ...)                                           \
  switch (D) {                                                         \
    case 64: { constexpr int HD = 64; __VA_ARGS__; } break;            \
    case 128: { constexpr int HD = 128; __VA_ARGS__; } break;          \
    default: return MM_ERR_UNSUPPORTED;                                \
  }

extern "C" int mm_qk_norm_bwd_blocks(int T) { return T <= 0 ? 0 : (T + QKN_BWD_ROWS_PER_BLOCK - 1) / QKN_BWD_ROWS_PER_BLOCK; }

extern "C" int mm_qk_norm_rope_fwd(int dtype, const void* x, int ld_in, int T, int Hq, int Hkv, int D, const void* w_q, const void* w_k,
                                   float eps, const float* cos_t, const float* sin_t, void* out, int ld_out, float* rstd, void* stream) {
  if (!x || !w_q || !w_k || !cos_t || !sin_t || !out || T < 0 || Hq <= 0 || Hkv <= 0 || D <= 0) return MM_ERR_ARG;
  if (dtype != MM_BF16 && dtype != MM_F32) return MM_ERR_UNSUPPORTED;
  if (D != 64 && D != 128) return MM_ERR_UNSUPPORTED;
  const int nh = Hq + Hkv;
  if (ld_in < nh * D || ld_out < nh * D || (out == x && ld_out != ld_in)) return MM_ERR_ARG;
  const int vn = dtype == MM_BF16 ? 8 : 4;
  if ((ld_in % vn) || (ld_out % vn) || !mm_aligned16(x) || !mm_aligned16(out) || !mm_aligned16(w_q) || !mm_aligned16(w_k)) return MM_ERR_ALIGN;
  if (T == 0) return MM_OK;
  const int64_t total = (int64_t)T * nh * (D / 2 / vn);
  dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MM_BF16) {
    QKN_DISPATCH(D, hipLaunchKernelGGL((qk_norm_rope_fwd_kernel<bf16, HD>), grid, block, 0, s, (const bf16*)x, ld_in, T, Hq, Hkv,
                                       (const bf16*)w_q, (const bf16*)w_k, eps, cos_t, sin_t, (bf16*)out, ld_out, rstd));
  } else {
    QKN_DISPATCH(D, hipLaunchKernelGGL((qk_norm_rope_fwd_kernel<float, HD>), grid, block, 0, s, (const float*)x, ld_in, T, Hq, Hkv,
                                       (const float*)w_q, (const float*)w_k, eps, cos_t, sin_t, (float*)out, ld_out, rstd));
  }
  MM_CHECK_LAUNCH();
  return MM_OK;
}

extern "C" int mm_qk_norm_rope_bwd(int dtype, const void* dqk, int ld_dqk, const void* x, int ld_x, int T, int Hq, int Hkv, int D,
                                   const void* w_q, const void* w_k, const float* rstd, const float* cos_t, const float* sin_t, void* dx,
                                   int ld_dx, float* dwq_partial, float* dwk_partial, void* stream) {
  if (!dqk || !x || !w_q || !w_k || !rstd || !cos_t || !sin_t || !dx || T < 0 || Hq <= 0 || Hkv <= 0 || D <= 0) return MM_ERR_ARG;
  if (!dwq_partial != !dwk_partial) return MM_ERR_ARG;
  if (dtype != MM_BF16 && dtype != MM_F32) return MM_ERR_UNSUPPORTED;
  if (D != 64 && D != 128) return MM_ERR_UNSUPPORTED;
  const int nh = Hq + Hkv;
  if (ld_dqk < nh * D || ld_x < nh * D || ld_dx < nh * D) return MM_ERR_ARG;
  const int vn = dtype == MM_BF16 ? 8 : 4;
  if ((ld_dqk % vn) || (ld_x % vn) || (ld_dx % vn) || !mm_aligned16(dqk) || !mm_aligned16(x) || !mm_aligned16(dx) || !mm_aligned16(w_q) ||
      !mm_aligned16(w_k))
    return MM_ERR_ALIGN;
  if (T == 0) return MM_OK;
  dim3 grid((unsigned)mm_qk_norm_bwd_blocks(T)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MM_BF16) {
    QKN_DISPATCH(D, hipLaunchKernelGGL((qk_norm_rope_bwd_kernel<bf16, HD>), grid, block, 0, s, (const bf16*)dqk, ld_dqk, (const bf16*)x, ld_x, T,
                                       Hq, Hkv, (const bf16*)w_q, (const bf16*)w_k, rstd, cos_t, sin_t, (bf16*)dx, ld_dx, dwq_partial, dwk_partial));
  } else {
    QKN_DISPATCH(D, hipLaunchKernelGGL((qk_norm_rope_bwd_kernel<float, HD>), grid, block, 0, s, (const float*)dqk, ld_dqk, (const float*)x, ld_x,
                                       T, Hq, Hkv, (const float*)w_q, (const float*)w_k, rstd, cos_t, sin_t, (float*)dx, ld_dx, dwq_partial,
                                       dwk_partial));
  }
  MM_CHECK_LAUNCH();
  return MM_OK;
}

extern "C" int mm_qk_norm_rope_append(int dtype, void* x, int T, int Hq, int Hkv, int D, int ld, const void* w_q, const void* w_k, float eps,
                                      const float* cos_t, const float* sin_t, void* kdst, void* vdst, int64_t dstride, void* stream) {
  if (!x || !w_q || !w_k || !cos_t || !sin_t || !kdst || !vdst || T < 0 || Hq <= 0 || Hkv <= 0 || D <= 0) return MM_ERR_ARG;
  if (dtype != MM_BF16 && dtype != MM_F32) return MM_ERR_UNSUPPORTED;
  if (D != 64 && D != 128) return MM_ERR_UNSUPPORTED;
  const int nh = Hq + 2 * Hkv;
  if (ld < nh * D || dstride < (int64_t)Hkv * D) return MM_ERR_ARG;
  const int vn = dtype == MM_BF16 ? 8 : 4;
  if ((ld % vn) || (dstride % vn) || !mm_aligned16(x) || !mm_aligned16(kdst) || !mm_aligned16(vdst) || !mm_aligned16(w_q) || !mm_aligned16(w_k))
    return MM_ERR_ALIGN;
  if (T == 0) return MM_OK;
  const int64_t total = (int64_t)T * nh * (D / 2 / vn);
  dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MM_BF16) {
    QKN_DISPATCH(D, hipLaunchKernelGGL((qk_norm_rope_append_kernel<bf16, HD>), grid, block, 0, s, (bf16*)x, ld, T, Hq, Hkv, (const bf16*)w_q,
                                       (const bf16*)w_k, eps, cos_t, sin_t, (bf16*)kdst, (bf16*)vdst, dstride));
  } else {
    QKN_DISPATCH(D, hipLaunchKernelGGL((qk_norm_rope_append_kernel<float, HD>), grid, block, 0, s, (float*)x, ld, T, Hq, Hkv, (const float*)w_q,
                                       (const float*)w_k, eps, cos_t, sin_t, (float*)kdst, (float*)vdst, dstride));
  }
  MM_CHECK_LAUNCH();
  return MM_OK;
}
