// GEMM launch policy: which kernel a problem runs on, on what grid and with which schedule.  gemm_plan is a pure function of the
// problem's facts, the option switches and the CU count: no HIP, no allocation, no environment.  mm_gemm.hip launches what it
// returns and mm_gemm_plan (mm_hip.h) reports it, so a policy change is an edit of this file and a diff of tests/golden/gemm_plan.jsonl.
#pragma once
#include <stdint.h>

#include "../../include/mm_hip.h"

// default LDS-DMA tile when the 256-wide tiles fill the chip: 1 = 256x128 (3-stage ring), 2 = 256x256 (2 stages)
#ifndef MM_DEFAULT_DMA_VARIANT
#define MM_DEFAULT_DMA_VARIANT(tiles256) ((tiles256) >= GEMM_FILL_TILES ? 2 : 1)
#endif
// schedules of gen_gemm_w4.py the 4-wave kernel's plain instantiations are built with beside schedule 1: X(schedule, the other arguments)
#ifdef MM_W4_DIAG
#define MM_W4_SCHEDS(X, ...) X(2, __VA_ARGS__) X(3, __VA_ARGS__) X(4, __VA_ARGS__) X(5, __VA_ARGS__) X(6, __VA_ARGS__) X(7, __VA_ARGS__) X(104, __VA_ARGS__) X(105, __VA_ARGS__) X(111, __VA_ARGS__) X(112, __VA_ARGS__) X(113, __VA_ARGS__) X(114, __VA_ARGS__) X(115, __VA_ARGS__) X(117, __VA_ARGS__) X(121, __VA_ARGS__)
#else
#define MM_W4_SCHEDS(X, ...) X(4, __VA_ARGS__) X(6, __VA_ARGS__) X(7, __VA_ARGS__)
#endif

constexpr int MM_EPI_SWIGLU_BWD = 1 << 20;   // internal epilogue flag (mm_gemm_swiglu_bwd), not part of the ABI enum
constexpr int MM_EPI_ACTS = MM_EPI_GELU_ERF | MM_EPI_QUICK_GELU | MM_EPI_GELU_TANH;

// the mm_set_option switches of the GEMM family (defaults = what ships)
struct GemmOptions {
  int persist = 1;          // walk tiles with resident workgroups
  int kernel = 0;           // 0 auto, 1 v1 (128x128 register staged), 2..6 LDS-DMA tiles 256x128, 256x256, 128x128, 64x128, 64x64
  int kernel_env = 0;       // MM_GEMM_KERNEL=v1|dma|big as a `kernel` value: used while `kernel` is 0 (A/B benchmarking)
  int tail = 1;             // cut the tiles of a less-than-half-full last round into 256x128 halves (persistent 256x256 grid)
  int skinny = 1;           // M <= 16 NT problems (decode) on the weight-streaming kernels
  int gemv_stream = 1;      // ... in the ring-buffered form (gemv_stream_kernel); 0 = gemm_skinny_kernel (A/B)
  int gemv_nt = 0;          // non-temporal policy on the decode kernels' weight loads (A/B: tools/gemv_bench.py)
  int gemv_wgs = 0;         // persistent workgroups per CU of gemv_stream_kernel (0 = what fits: 2, or 1 with a large x)
  int small = -1;           // experiments: force the DMA variant for problems that do not fill the chip (-1 = heuristic)
  int epi_pipe = 1;         // pipelined, branch-free epilogue of the plain / SwiGLU-backward LDS-DMA kernels
  int issue_waves = 4;      // waves that issue the 256x256 kernel's DMA (4 staggers the two waves of each SIMD)
  int w4 = 1;               // 256x256 tiles on the 4-wave hand-scheduled kernel: 0 = the 8-wave kernel (A/B; MM_GEMM_W4 gives the
                            // initial value), 1 = the shipped schedule, n > 1 = another schedule of MM_W4_SCHEDS
  int w4_big = 4;           // 4 = the split-barrier schedule 4 for operands that stream from HBM, 1 = schedule 1 everywhere
  int w4_group_m = 8;       // experiment: GROUP_M of the 4-wave kernel's tile order
  int w4_stream = 1;        // 4-wave kernel: wait-free plain epilogue (0 = gemm_epilogue_plain_pipe, A/B)
  int w4_shuffle = 0;       // GemmArgs::shuffle (measured equal to the LDS form within +-0.5 %: DESIGN.md section 4)
  int w4_diag_epi = 0;      // MM_W4_DIAG builds: GemmArgs::diag_epi
  int w4_stagger_slots = 4, w4_stagger = 0;      // experiment: see GemmArgs::stagger
  int w4_rowmajor = 1;      // 4-wave kernel: row-major (LDS-transposed, 16-byte) plain epilogue; 0 = the accumulator-layout one (A/B)
};

enum GemmKind { GEMM_PLAIN = 0, GEMM_ACT_FWD = 1, GEMM_SWIGLU_FWD = 2, GEMM_ROPE_FWD = 3, GEMM_SWIGLU_BWD = 4 };
// low four address bits of the pointers the policy looks at, one nibble each (a grouped call: the OR over its problems)
enum { GEMM_PTR_A = 0, GEMM_PTR_B = 4, GEMM_PTR_C = 8, GEMM_PTR_BIAS = 12, GEMM_PTR_RESIDUAL = 16, GEMM_PTR_AUX = 20, GEMM_PTR_C2 = 24 };
struct GemmProblem {
  int dtype, layout;
  int kind;                 // GemmKind: act_fwd keeps the pre-activation (C2), swiglu_fwd has N = 2 swi_I
  int groups;               // 0 = a stand-alone call, else the problems of one grouped launch
  int M, N, K, lda, ldb, ldc, ldr, ldaux;
  int epi;                  // MM_EPI_* (| MM_EPI_SWIGLU_BWD)
  int swi_I;
  unsigned ptr_bits;
  bool misaligned(int which, int mask) const { return ((ptr_bits >> which) & mask) != 0; }
};

enum GemmFamily { GEMM_FAM_NONE = -1, GEMM_FAM_V1 = 0, GEMM_FAM_DMA = 1, GEMM_FAM_W4 = 2, GEMM_FAM_SKINNY = 3, GEMM_FAM_GEMV = 4, GEMM_FAM_F32 = 5 };
constexpr int GEMM_LAST_UNCHANGED = -2;      // GemmPlan::last_kernel: the call leaves "gemm_last_kernel" as it was
// Everything about one launch, as ints (mm_gemm_plan copies the struct out as it stands).  Template arguments t[] per family:
//   v1 {A_KC, B_KC}   dma {A_KC, B_KC, BM, BN, WGM, STAGES, ISSUE_WAVES, EK}   w4 {A_KC, B_KC, EK, SCHED}   gemv {MODE, NORM, NT}   f32 {LAYOUT}
struct GemmPlan {
  int rc = MM_OK;           // what the call returns before launching
  int last_kernel = GEMM_LAST_UNCHANGED;      // "gemm_last_kernel" after the call (ids: mm_hip.h)
  int family = GEMM_FAM_NONE;
  int t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int grid_x = 0, grid_y = 0, block = 0, lds = 0;
  // the GemmArgs fields of the same names
  int nbm = 0, nbn = 0, tail = 0, pipe = 0, stagger = 0, stagger_slots = 0, diag_epi = 0, shuffle = 0, group_m = 0, stream_epi = 0, rowmajor = 0;
  GemmPlan& launch(int fam, int last, int64_t gx, int blk, int ldsb, int t0 = 0, int t1 = 0, int t2 = 0, int t3 = 0, int t4 = 0, int t5 = 0,
                   int t6 = 0, int t7 = 0) {
    family = fam; last_kernel = last; grid_x = (int)gx; block = blk; lds = ldsb;
    t[0] = t0; t[1] = t1; t[2] = t2; t[3] = t3; t[4] = t4; t[5] = t5; t[6] = t6; t[7] = t7;
    return *this;
  }
};
static_assert(sizeof(GemmPlan) == MM_GEMM_PLAN_INTS * sizeof(int), "mm_hip.h documents the layout of mm_gemm_plan's output");

// ---- the M <= 16 weight-streaming kernel (plain mm_gemm rows and the mm_decode_* fusions) ---------------------------------------
// x rows are staged in LDS beside gemv_stream_kernel's STATIC arrays (red: 2 x 8 x 4 x 64 floats = 16 384 B, nred: 128 B) in the
// 160 KB of a CU: 143 KB leaves 896 B of slack.  kernels.decode_fits mirrors the number.
constexpr int64_t GEMV_X_LDS_MAX = 143 * 1024;
static_assert(GEMV_X_LDS_MAX + 2 * 8 * 4 * 64 * 4 + 8 * 4 * 4 <= 160 * 1024, "x + static reduction scratch must fit the CU's LDS");
inline bool gemv_stream_fits(int M, int K) { return (K & 7) == 0 && (int64_t)M * K * 2 <= GEMV_X_LDS_MAX; }

// persistent grid over `nblk` 16-row blocks of W: as many workgroups as the chip holds at once (2 per CU by registers, 1 when x
// takes most of the LDS)
struct GemvGrid { int per_cu; unsigned grid; int lds; };
inline GemvGrid gemv_grid(int M, int K, unsigned nblk, const GemmOptions& o, int ncu) {
  const int lds = M * K * 2, per_cu = o.gemv_wgs > 0 ? o.gemv_wgs : (((int64_t)lds + 17 * 1024) * 2 <= 160 * 1024 ? 2 : 1);
  const unsigned cap = (unsigned)(ncu * per_cu);
  return {per_cu, nblk < cap ? nblk : cap, lds};
}

// ---- tiles -------------------------------------------------------------------------------------------------------------------------
// A problem whose 256x128 tiles number GEMM_FILL_TILES or more fills the chip with 256-wide tiles.  Smaller ones (ViT-L/14 on 4
// images = 1028 rows, the projector) are latency-bound, so the tile is chosen by how many workgroups it yields (tools/gemm_bench.py
// --small): 64x128 wins up to 96 tiles of 128x128, the 128x128 LDS-DMA kernel up to 320, beyond that the register-staged 128x128
// kernel at 2 workgroups per CU.  A grouped launch counts the tiles of all its problems.
constexpr int64_t GEMM_FILL_TILES = 192;
inline int gemm_small_variant(const GemmProblem& p, const GemmOptions& o) {
  if (o.small >= 0) return o.small;
  const int64_t t = (int64_t)(p.groups ? p.groups : 1) * ((p.M + 127) / 128) * ((p.N + 127) / 128);
  return t <= 96 ? 4 : (t <= 320 ? 3 : 0);
}
constexpr int64_t GEMM_HBM_DIM = 14336;      // a dimension this long streams its operand from beyond the Infinity Cache

inline int gemm_w4_sched(int asked) {        // the schedule the 4-wave kernel is instantiated with for "gemm_w4" = asked
  switch (asked) {
#define MM_W4_SCHED_CASE(S, ...) case S:
    MM_W4_SCHEDS(MM_W4_SCHED_CASE, ~)
#undef MM_W4_SCHED_CASE
    return asked;
    default: return 1;
  }
}

inline GemmPlan gemm_plan(const GemmProblem& p, const GemmOptions& o, int ncu) {
  constexpr int64_t LIM32 = 0xFFFFFFFFll;
  const int M = p.M, N = p.N, K = p.K, layout = p.layout, epi = p.epi;
  const bool grouped = p.groups > 0, acts = (epi & MM_EPI_ACTS) != 0;
  const bool swi = p.kind == GEMM_SWIGLU_FWD, rope = p.kind == GEMM_ROPE_FWD, swi_bwd = (epi & MM_EPI_SWIGLU_BWD) != 0;
  const int a_kc = layout != MM_GEMM_TN, b_kc = layout == MM_GEMM_NT;
  const auto fail = [](int rc, int last_kernel) { GemmPlan f; f.rc = rc; f.last_kernel = last_kernel; return f; };
  GemmPlan pl;
  pl.pipe = o.epi_pipe;
  pl.grid_y = grouped ? p.groups : 1;
  if (p.dtype == MM_F32) {                    // parity only: 64x64 tiles, one each
    pl.nbm = (M + 63) / 64;
    pl.nbn = (N + 63) / 64;
    if ((int64_t)pl.nbm * pl.nbn > 0x7FFFFFFF) return fail(MM_ERR_ARG, grouped ? GEMM_LAST_UNCHANGED : 30);
    return pl.launch(GEMM_FAM_F32, 30, pl.nbm * pl.nbn, 256, 0, layout);
  }
  if (p.dtype != MM_BF16) return fail(MM_ERR_UNSUPPORTED, GEMM_LAST_UNCHANGED);
  // a stand-alone bf16 call that does not launch reports kernel 0 (or the kernel it had chosen); a grouped one leaves the id alone
  const int no_launch = grouped ? GEMM_LAST_UNCHANGED : 0;
  if ((p.lda & 7) || (p.ldb & 7) || (p.ldc & 3) || ((epi & MM_EPI_RESIDUAL) && (p.ldr & 3))) return fail(MM_ERR_ALIGN, no_launch);
  if (p.misaligned(GEMM_PTR_A, 15) || p.misaligned(GEMM_PTR_B, 15) || p.misaligned(GEMM_PTR_C, 7)) return fail(MM_ERR_ALIGN, no_launch);
  const int forced = o.kernel ? o.kernel : o.kernel_env;

  // decode (M <= 16, NT): stream W once.  Such problems fill the chip on their own: no grouped form.
  if (forced == 0 && o.skinny && layout == MM_GEMM_NT && M <= 16) {
    if (grouped) return fail(MM_ERR_UNSUPPORTED, no_launch);
    if (!swi && !rope && (int64_t)16 * p.lda * 2 < LIM32 && (int64_t)16 * p.ldb * 2 < LIM32) {
      const unsigned nblk = (unsigned)((N + 15) / 16);
      if (!o.gemv_stream || !gemv_stream_fits(M, K) || (int64_t)N * p.ldb * 2 >= LIM32) return pl.launch(GEMM_FAM_SKINNY, 20, nblk, 512, 0);
      const GemvGrid gg = gemv_grid(M, K, nblk, o, ncu);       // the ring-buffered form (same bits)
      pl.pipe = 0;                            // takes SkinnyArgs: no GemmArgs field
      return pl.launch(GEMM_FAM_GEMV, 21, gg.grid, 512, gg.lds, 0, 0, o.gemv_nt);
    }
  }

  // the DMA kernels address a K-strided operand with 32-bit byte offsets over the whole matrix, and (pipelined epilogues) one wave
  // tile of C / residual / aux with 32-bit byte offsets: 128 rows of the largest leading dimension
  const int64_t ldmax = p.ldc > p.ldr ? (p.ldc > p.ldaux ? p.ldc : p.ldaux) : (p.ldr > p.ldaux ? p.ldr : p.ldaux);
  const bool fits32 = ldmax * 128 * 2 + (int64_t)N * 2 < 0x7FFFFFFFll &&
                      (layout == MM_GEMM_NT || ((int64_t)K * p.ldb * 2 < LIM32 && (layout != MM_GEMM_TN || (int64_t)K * p.lda * 2 < LIM32)));
  const int64_t tiles_128 = (int64_t)((M + 255) / 256) * ((N + 127) / 128);
  const int64_t tiles_256 = (int64_t)((M + 255) / 256) * ((N + 255) / 256);
  int variant = 0;   // 0 = v1 (128x128 register staged); DMA tiles: 1 = 256x128, 2 = 256x256, 3 = 128x128, 4 = 64x128, 5 = 64x64
  if (swi || rope) {                          // the fused gate|up / RoPE tiles are defined on the 256x256 kernels only
    if (grouped || !fits32) return fail(MM_ERR_UNSUPPORTED, no_launch);
    variant = 2;
  } else if (p.kind == GEMM_ACT_FWD) {        // the kept pre-activation is compiled into the small-tile DMA kernels only
    if (!fits32 || forced == 1) return fail(MM_ERR_UNSUPPORTED, no_launch);
    variant = (forced >= 4 && forced <= 6) ? forced - 1 : gemm_small_variant(p, o);
    if (variant < 3) variant = 3;             // a problem that would take a 256-wide tile: 128x128 (the caller may prefer the separate launches)
  } else if (fits32) {
    if (forced >= 2 && forced <= 6) variant = forced - 1;
    else if (forced == 0 && tiles_128 >= GEMM_FILL_TILES) variant = MM_DEFAULT_DMA_VARIANT(tiles_256);
    else if (forced == 0) variant = gemm_small_variant(p, o);
  }
  if (grouped) {
    // only the small LDS-DMA tiles have a grouped form.  Where a stand-alone call takes the register-staged 128x128 kernel (more
    // than 320 tiles in the batch) the LDS-DMA kernel of the same tile runs instead (same bits), except past the 32-bit offsets
    // and where that kernel was asked for by name
    if (swi_bwd || (acts && layout != MM_GEMM_NT) || variant == 1 || variant == 2) return fail(MM_ERR_UNSUPPORTED, no_launch);
    if (variant == 0 && fits32 && forced != 1) variant = 3;
    if (variant == 0) return fail(MM_ERR_UNSUPPORTED, no_launch);
  }

  static constexpr int TBM[6] = {128, 256, 256, 128, 64, 64}, TBN[6] = {128, 128, 256, 128, 128, 64}, WGM[6] = {0, 4, 2, 2, 2, 2};
  const int bm = TBM[variant], bn = TBN[variant];
  pl.nbm = (M + bm - 1) / bm;
  pl.nbn = swi ? p.swi_I / 128 : (N + bn - 1) / bn;
  const int64_t nwg = (int64_t)pl.nbm * pl.nbn;
  if (nwg > 0x7FFFFFFF) return fail(MM_ERR_ARG, no_launch);
  if (variant == 0) return pl.launch(GEMM_FAM_V1, 0, nwg, 256, 4 * 128 * 64 * 2, a_kc, b_kc);      // two stages of an A and a B tile
  // persistent: one resident workgroup per CU walks the tiles (of its problem); otherwise one tile each
  int64_t nblk = o.persist ? (nwg < ncu ? nwg : ncu) : nwg;
  // wave quantisation: a last round at most half full has its 256x256 tiles cut into 256x128 halves (GemmArgs::tail)
  const int64_t rem = o.persist ? nwg % ncu : 0;
  const bool w4 = o.w4 && variant == 2 && K >= 192 && !acts;      // the 4-wave kernel: whole K-steps in flight, the epilogue kinds it instantiates
  if (o.tail && variant == 2 && !swi && !rope && !(w4 && swi_bwd) && rem > 0 && 2 * rem <= ncu) {
    pl.tail = (int)rem;
    nblk = nwg >= ncu ? ncu : 2 * rem;
  }
  // epilogue kind = kernel instantiation: the fused ones exist for the layout their entry point uses only
  const int ek = rope ? 4 : swi ? 3 : swi_bwd ? 2 : acts ? 1 : 0;
  if ((ek >= 3 && layout != MM_GEMM_NT) || (ek == 2 && layout != MM_GEMM_NN)) return fail(MM_ERR_ARG, w4 ? 10 : variant);
  if (!w4) {
    if (acts && layout != MM_GEMM_NT) return fail(MM_ERR_UNSUPPORTED, variant);      // activation: NT (mm_gemm / mm_gemm_act_fwd)
    const int issue = variant == 1 ? 8 : (variant == 2 ? o.issue_waves : 4);
    return pl.launch(GEMM_FAM_DMA, variant, nblk, 512, 2 * (bm + bn) * 64 * 2, a_kc, b_kc, bm, bn, WGM[variant], 2, issue, ek);
  }
  // schedule 1 everywhere (one barrier per K-step), except -- "gemm_w4_big" = 4 -- on operands that stream from HBM (a wide N or a
  // long K): there the split-barrier schedule 4 (a DMA piece gets 105-168 MFMAs to land instead of 68-128) measured +3...+9 %
  // (tools/w4_check.py --scheds), while on MALL-resident 4096-sized operands it costs 3 %
  const bool big = o.w4_big == 4 && o.w4 == 1 && (N >= GEMM_HBM_DIM || K >= GEMM_HBM_DIM);
  const int sched = ek == 4 ? 1 : ek ? (big ? 4 : 1) : gemm_w4_sched(big && layout != MM_GEMM_TN ? 4 : o.w4);
  pl.stagger = o.w4_stagger; pl.stagger_slots = o.w4_stagger_slots; pl.diag_epi = o.w4_diag_epi;
  pl.shuffle = o.w4_shuffle; pl.group_m = o.w4_group_m; pl.stream_epi = o.w4_stream;
  // row-major (16-byte) stores where alignment allows; mm_gemm_swiglu_fwd's are 8-byte ones, checked at the entry point
  pl.rowmajor = o.w4_rowmajor &&
                (swi || ((N & 7) == 0 && (p.ldc & 7) == 0 && !p.misaligned(GEMM_PTR_C, 15) &&
                         (!(epi & MM_EPI_RESIDUAL) || ((p.ldr & 7) == 0 && !p.misaligned(GEMM_PTR_RESIDUAL, 15))) &&
                         (!(epi & MM_EPI_BIAS) || !p.misaligned(GEMM_PTR_BIAS, 15)) &&
                         (!swi_bwd || ((p.ldaux & 7) == 0 && !p.misaligned(GEMM_PTR_AUX, 15)))));
  // LDS: the ring (128 KB) + 8 KB per wave for the row-major epilogue's transposition
  return pl.launch(GEMM_FAM_W4, 10, nblk, 256, 160 * 1024, a_kc, b_kc, ek, sched);
}
