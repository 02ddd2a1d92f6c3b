// MXFP8 x MXFP8 GEMM on gfx950's block-scaled MFMA (include/mm_hip.h: mm_gemm_mx8, mm_gemm_mx8_supported; the format and the buffer
// layout: mm_mxfp8.h).  C[m,n] = bf16( sum_k A'[m,k] W'[n,k] (+ bias[n]) (+ residual[m,n]) ), A' and W' the matrices mm_dequant_mxfp8
// returns for the two packed buffers; fp32 accumulation in a fixed order, one rounding at the store.
//
// INSTRUCTION.  v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz = blgp = 0 (e4m3 on both sides).  The lane maps, MEASURED on the MI355X
// with one-hot operands and a different scale in every lane (both operands alike; g = l >> 4):
//   elements: lane l holds row (l & 15); its bytes 0..15 are k = 16 g .. 16 g + 15 and its bytes 16..31 are k = 64 + 16 g .. + 15
//             (two 16x16x64 halves side by side -- NOT 32 consecutive k);
//   scales:   the E8M0 byte of (row r, block b = k / 32) is taken from lane r + 16 b (byte 0 of the VGPR under opsel 0).
// So a lane's elements belong to the blocks g >> 1 and 2 + (g >> 1) while its scale byte is block g's.  The result has the 16x16 C/D
// map of the bf16 forms.  As in the bf16 kernels the WEIGHT fragment goes into the first operand, so that a lane ends with 4
// consecutive n of one m: D[4 (l >> 4) + e][l & 15] = C[m = l & 15][n = 4 (l >> 4) + e].
//
// LAYOUT.  A packed row is 8 runs of sper step slots (mm_mxfp8.h); slot pairs are 64 contiguous bytes and a row's slots, padding
// included, follow each other, so a row is ONE contiguous string of 8 * sper * 32 bytes and its scale bytes one of 8 * sper.  The
// kernel walks ALL of it, 4 slots (128 bytes, one aligned scale dword) per stage: a padding slot holds zeros under scale 2^0 and adds
// nothing, which is what lets every K % 128 == 0 through (the widths without padding -- per % 4 == 0 -- do no wasted work).  The sum
// over k does not care in which order the slots come, only that A and W agree, and both are packed for the same K.
// A 16-byte piece of a slot pair holds 8 bytes of the even and 8 of the odd slot (k-chunk kc of both), so a lane's 16 bytes of a
// block are two 8-byte reads, 16 bytes apart: four ds_read_b64 per fragment.
//
// TILE.  256 x 256 per workgroup of 8 waves (2 x 4, a wave owns 128 x 64 = 8 x 4 MFMA tiles), 128 k per stage: 32 KiB of A, 32 KiB of
// W and 2 KiB of scale dwords, two stages in a ring.  All of it arrives by LDS-DMA: a 16-byte DMA writes lane l's piece to
// (wave-uniform base) + 16 l, so a DMA fills 8 rows of 128 bytes and the PER-LANE GLOBAL ADDRESS chooses which piece of the row goes
// to which place: piece c of row r sits at position c ^ ((r >> 1) & 7), which spreads the 16 rows of a fragment read over the banks
// (a slot still fills only one 8-byte half of every 16-byte unit: the 2-way conflict that is left is measured in profiles/r07_mx8_prefill.md).
// The scales come with 4-byte DMAs (one per wave and stage: the stage's dword of 64 rows).  One raw barrier per stage: wait for the
// own DMAs of this stage, barrier, issue the next stage into the other half, multiply.  Rows past M / N are never read: the buffer
// descriptors end at the last real row and the hardware range check writes zeros.
#include "mm_mxfp8.h"

typedef int i32x8 __attribute__((ext_vector_type(8)));

__attribute__((visibility("hidden"))) void mm_gemm_note_last_kernel(int id);      // mm_gemm.hip ("gemm_last_kernel")

namespace {

constexpr int MX_BM = 256, MX_BN = 256, MX_STAGE_K = 128;
constexpr int MX_A_BYTES = MX_BM * MX_STAGE_K, MX_B_BYTES = MX_BN * MX_STAGE_K, MX_SC_BYTES = (MX_BM + MX_BN) * 4;
constexpr int MX_STAGE_BYTES = MX_A_BYTES + MX_B_BYTES + MX_SC_BYTES;
constexpr int MX_LDS = 2 * MX_STAGE_BYTES;                                       // 135 168 of the 163 840 bytes
constexpr int MX_MREP = 8, MX_NREP = 4;

struct Mx8GemmArgs {
  const unsigned char* A;
  const unsigned char* W;
  const bf16* bias;
  const bf16* residual;
  bf16* C;
  Mx8Layout La, Lw;
  int M, N, nstage, ldc, ldr, nbm, nbn;
};

// 4-byte LDS-DMA: lane l's dword lands at lds_addr + 4 * l (see lds_dma16 in mm_common.h)
__device__ __forceinline__ void lds_dma4(const SRsrc& r, unsigned voff, unsigned lds_addr) {
  u32x4 d = {r.w0, r.w1, r.w2, r.w3};
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 4\n\t"
      "buffer_load_dword %1, %3, 0 offen lds\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(lds_addr), "s"(d)
      : "memory");
}

// blocks b and b + 8 share an XCD: each XCD gets a contiguous run of tile ids, and inside it 8 row tiles walk the column tiles
// together, so a W tile is fetched once per 8 A tiles
__device__ __forceinline__ void mx8_tile_of(int bid, int nbm, int nbn, int& pm, int& pn) {
  const int total = nbm * nbn;
  const int xcd = bid & 7, idx = bid >> 3, q = total >> 3, r = total & 7;
  const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  const int width = 8 * nbn, grp = id / width, first = grp * 8, gsz = min(nbm - first, 8), in = id - grp * width;
  pm = first + in % gsz;
  pn = in / gsz;
}

__global__ __launch_bounds__(512) void gemm_mx8_kernel(Mx8GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wm = w >> 2, wn = w & 3;
  int pm, pn;
  mx8_tile_of((int)blockIdx.x, g.nbm, g.nbn, pm, pn);
  const int m0 = pm * MX_BM, n0 = pn * MX_BN;
  const unsigned lds0 = (unsigned)(uintptr_t)LDS_PTR(char, smem);

  // ---- this wave's share of a stage's DMAs: waves 0-3 bring the A rows 64 (w & 3) .. + 63, waves 4-7 the W rows
  const bool is_a = w < 4;
  const unsigned char* base = is_a ? g.A : g.W;
  const Mx8Layout L = is_a ? g.La : g.Lw;
  const int row0 = is_a ? m0 : n0, rows = (is_a ? g.M : g.N) - row0;            // rows > 0: the tile exists
  const int64_t rowb = mx8_elem_off(L, 8, 0, 0);                                // bytes of one row's slots: 8 runs
  const int srow = 8 * L.sper;                                                   // and of its scale bytes
  const SRsrc re = make_srsrc(base + mx8_elem_off(L, (int64_t)row0 * 8, 0, 0), (int64_t)rows * rowb);
  const SRsrc rs = make_srsrc(base + L.scale_off + (int64_t)row0 * srow, (int64_t)rows * srow);
  unsigned offe[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int r = (w & 3) * 64 + q * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    offe[q] = (unsigned)r * (unsigned)rowb + (unsigned)c * 16u;
  }
  const unsigned offs = (unsigned)((w & 3) * 64 + lane) * (unsigned)srow;
  auto issue = [&](int t, int stage) {
    const unsigned st = lds0 + (unsigned)(stage * MX_STAGE_BYTES);
#pragma unroll
    for (int q = 0; q < 8; ++q) lds_dma16(re, offe[q] + (unsigned)t * 128u, st + (unsigned)((w * 8 + q) * 1024));
    lds_dma4(rs, offs + (unsigned)t * 4u, st + (unsigned)(MX_A_BYTES + MX_B_BYTES + w * 256));
  };

  // ---- this lane's place in a 16-row fragment: row l & 15, group g = l >> 4.  Its first 16 bytes are the k-half g & 1 of block
  // g >> 1 (the stage's slot g >> 1: slot pair 0, the even / odd 8 bytes of the pieces kc = 2 (g & 1), + 1), its last 16 bytes the
  // same of block 2 + (g >> 1) (slot pair 1); its scale byte is block g's (read at `so`).
  const int lr = lane & 15, kb = lane >> 4;
  unsigned fo[4];
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const int piece = (x >> 1) * 4 + (kb & 1) * 2 + (x & 1);
    fo[x] = (unsigned)(lr * 128 + ((piece ^ ((lr >> 1) & 7)) * 16) + (kb >> 1) * 8);
  }
  const unsigned so = (unsigned)(MX_A_BYTES + MX_B_BYTES + lr * 4 + kb);
  auto frag = [&](const char* tile, int rep) {                                   // tile: the A or W half of a stage; 16 rows per rep
    const char* p = tile + rep * 16 * 128;
    const u32x2 p0 = *LDS_PTR(const u32x2, p + fo[0]), p1 = *LDS_PTR(const u32x2, p + fo[1]);
    const u32x2 p2 = *LDS_PTR(const u32x2, p + fo[2]), p3 = *LDS_PTR(const u32x2, p + fo[3]);
    return i32x8{(int)p0[0], (int)p0[1], (int)p1[0], (int)p1[1], (int)p2[0], (int)p2[1], (int)p3[0], (int)p3[1]};
  };

  f32x4 acc[MX_MREP][MX_NREP];
#pragma unroll
  for (int i = 0; i < MX_MREP; ++i)
#pragma unroll
    for (int j = 0; j < MX_NREP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  issue(0, 0);
  for (int t = 0; t < g.nstage; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                             // the 9 DMAs of stage t (nothing else is in flight)
    __builtin_amdgcn_s_barrier();                                                // ... of every wave; and all have left stage t - 1
    if (t + 1 < g.nstage) issue(t + 1, (t + 1) & 1);
    const char* cur = smem + (t & 1) * MX_STAGE_BYTES;
    i32x8 wf[MX_NREP];
    int wsc[MX_NREP];
#pragma unroll
    for (int j = 0; j < MX_NREP; ++j) {
      wf[j] = frag(cur + MX_A_BYTES, wn * MX_NREP + j);
      wsc[j] = *LDS_PTR(const unsigned char, cur + so + (MX_BM + (wn * MX_NREP + j) * 16) * 4);
    }
#pragma unroll
    for (int i = 0; i < MX_MREP; ++i) {
      const i32x8 af = frag(cur, wm * MX_MREP + i);
      const int asc = *LDS_PTR(const unsigned char, cur + so + (wm * MX_MREP + i) * 16 * 4);
#pragma unroll
      for (int j = 0; j < MX_NREP; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[j], af, acc[i][j], 0, 0, 0, wsc[j], 0, asc);
    }
  }

  // ---- epilogue: acc (+ bias) (+ residual) in fp32, one rounding; a lane holds C[m][n .. n + 3]
#pragma unroll
  for (int i = 0; i < MX_MREP; ++i) {
    const int m = m0 + (wm * MX_MREP + i) * 16 + lr;
    if (m >= g.M) continue;
#pragma unroll
    for (int j = 0; j < MX_NREP; ++j) {
      const int n = n0 + (wn * MX_NREP + j) * 16 + kb * 4;
      if (n >= g.N) continue;
      bf16* cp = g.C + (int64_t)m * g.ldc + n;
      const bf16* rp = g.residual ? g.residual + (int64_t)m * g.ldr + n : nullptr;
      const bool vec = n + 3 < g.N && (((uintptr_t)cp) & 7) == 0 && (((uintptr_t)rp) & 7) == 0;
      float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
      if (g.bias) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (n + e < g.N) v[e] += (float)g.bias[n + e];
      }
      if (vec) {
        if (rp) {
          const bf16x4 rv = *(const bf16x4*)rp;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += (float)rv[e];
        }
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (bf16)v[e];
        *(bf16x4*)cp = o;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (n + e < g.N) cp[e] = (bf16)(rp ? v[e] + (float)rp[e] : v[e]);
      }
    }
  }
}

}  // namespace

extern "C" int mm_gemm_mx8_supported(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return MM_ERR_ARG;
  if (K % MX_STAGE_K) return MM_ERR_UNSUPPORTED;
  if (K > (1 << 20)) return MM_ERR_UNSUPPORTED;                                 // 256 rows of a tile within the DMA's 32-bit offsets
  const int64_t tiles = (int64_t)((M + MX_BM - 1) / MX_BM) * ((N + MX_BN - 1) / MX_BN);
  if (tiles >= 0x7FFFFFFF) return MM_ERR_UNSUPPORTED;
  return MM_OK;
}

extern "C" int mm_gemm_mx8(int M, int N, int K, const void* packedA, const void* packedW, const void* bias, const void* residual, int ldr,
                           void* C, int ldc, int epi, void* stream) {
  if (epi & ~(MM_EPI_BIAS | MM_EPI_RESIDUAL)) return MM_ERR_UNSUPPORTED;
  const int rc = mm_gemm_mx8_supported(M, N, K);
  if (rc != MM_OK) return rc;
  if (!packedA || !packedW || !C || ldc < N) return MM_ERR_ARG;
  if ((epi & MM_EPI_BIAS) && !bias) return MM_ERR_ARG;
  if ((epi & MM_EPI_RESIDUAL) && (!residual || ldr < N)) return MM_ERR_ARG;
  if (!mm_aligned16(packedA) || !mm_aligned16(packedW) || (((uintptr_t)C) & 1) || (((uintptr_t)bias) & 1) || (((uintptr_t)residual) & 1))
    return MM_ERR_ALIGN;
  Mx8GemmArgs g;
  g.A = (const unsigned char*)packedA;
  g.W = (const unsigned char*)packedW;
  g.bias = (epi & MM_EPI_BIAS) ? (const bf16*)bias : nullptr;
  g.residual = (epi & MM_EPI_RESIDUAL) ? (const bf16*)residual : nullptr;
  g.C = (bf16*)C;
  g.La = mx8_layout(M, K);
  g.Lw = mx8_layout(N, K);
  g.M = M;
  g.N = N;
  g.nstage = 8 * g.La.sper / 4;                                                  // every slot of a row, 4 per stage
  g.ldc = ldc;
  g.ldr = ldr;
  g.nbm = (M + MX_BM - 1) / MX_BM;
  g.nbn = (N + MX_BN - 1) / MX_BN;
  auto kfn = gemm_mx8_kernel;
  if (hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, MX_LDS) != hipSuccess) {
    (void)hipGetLastError();
    return MM_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL(kfn, dim3((unsigned)(g.nbm * g.nbn)), dim3(512), MX_LDS, (hipStream_t)stream, g);
  MM_CHECK_LAUNCH();
  mm_gemm_note_last_kernel(23);
  return MM_OK;
}
