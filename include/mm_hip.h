/*
 * mm_hip.h -- C ABI of libmmhip.so: the MI355X (gfx950) kernels under the MultiMeditron
 * multimodal hot path  (modality encoder -> projector -> embed-splice -> LLM decoder, fwd+bwd).
 *
 * The reference (leagrieder/MultiMeditron) has no FFI: its operator boundary for this path is a
 * set of Python/torch calls.  Each entry point below replaces the torch/HF call(s) cited next to
 * it (paths under /root/reference/src/multimeditron/, `HF:` = transformers 5.15.0).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to a row-major buffer; no torch types cross the ABI
 *   - `stream` is a hipStream_t passed as void*; work is enqueued, never synchronised
 *   - nothing is allocated inside; the caller provides outputs and workspaces
 *   - return value: 0 = MM_OK, negative = error (mm_error_string); no exceptions, no aborts
 *   - dtype: MM_BF16 (storage bf16, fp32 accumulate) or MM_F32 (exact fp32; parity path)
 */
#ifndef MM_HIP_H
#define MM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { MM_BF16 = 0, MM_F32 = 1 } mm_dtype;

enum { MM_OK = 0, MM_ERR_ARG = -1, MM_ERR_ALIGN = -2, MM_ERR_UNSUPPORTED = -3, MM_ERR_LAUNCH = -4 };

/* GEMM operand layouts.  C is always [M,N] row-major (ldc). */
enum {
  MM_GEMM_NT = 0, /* A[M,K] (lda), B[N,K] (ldb): y = x W^T      -- nn.Linear forward            */
  MM_GEMM_NN = 1, /* A[M,K] (lda), B[K,N] (ldb): dx = dy W      -- nn.Linear input gradient     */
  MM_GEMM_TN = 2  /* A[K,M] (lda), B[K,N] (ldb): dW = dy^T x    -- nn.Linear weight gradient    */
};

/* GEMM epilogue flags (OR-ed) */
enum {
  MM_EPI_BIAS = 1,       /* + bias[N]                                      */
  MM_EPI_GELU_ERF = 2,   /* exact GELU (projectors/mlp.py:35,37)           */
  MM_EPI_QUICK_GELU = 4, /* x*sigmoid(1.702x) (HF:activations.py:117-123)  */
  MM_EPI_RESIDUAL = 8,   /* + residual[M,N] (ldr)                          */
  MM_EPI_ACCUMULATE = 16,/* C += result (gradient accumulation)            */
  MM_EPI_GELU_TANH = 32  /* tanh GELU (HF:activations.py gelu_pytorch_tanh; SigLIP MLP) */
};

/* most problems in one grouped launch (the *_batched entry points below) */
enum { MM_GROUP_MAX = 16 };

int mm_version(void);
const char* mm_error_string(int code);
/* tuning / A-B switches (benchmarks and the trainer): "gemm_persist" 0|1 (persistent one-workgroup-per-CU grid; the
 * trainer sets 0 under data parallelism), "gemm_kernel" 0 auto | 1 register-staged 128x128 | 2..6 LDS-DMA tiles 256x128,
 * 256x256, 128x128, 64x128, 64x64, "gemm_small" -1 auto | 0..5, "gemm_tail" 0|1 (half-tile last round), "gemm_skinny"
 * 0|1 (M <= 16 weight-streaming kernel), "gemm_issue_waves" 4|8 (how many of a workgroup's 8 waves
 * issue the LDS-DMA); round 4: "gemm_w4" 0 | 1 | n (256x256 tiles on the 4-wave
 * hand-scheduled kernel gemm_bf16_w4_kernel: 0 = the 8-wave kernel, 1 = the shipped schedule, n = another schedule of
 * csrc/gen_gemm_w4.py: 4 / 5 split barriers, 6 / 7 = 1 / 4 with an L2 prefetch), "gemm_w4_big" 4|1 (schedule 4 where N or K >= 14336: default), "gemm_w4_rowmajor" 0|1 (its row-major, LDS-transposed epilogues), "gemm_w4_stream" 0|1 (wait-free plain
 * epilogue in the accumulator layout), "gemm_w4_shuffle" (0; 1 = the plain epilogue by register lane exchange instead of the LDS round trip: bit-identical, measured equal),
 * "gemm_w4_group_m", "gemm_w4_stagger" / "gemm_w4_stagger_slots" (experiments), "gemm_epi_pipe" 0|1, "gemv_stream" 0|1, "gemv_nt" 0|1,
 * "gemv_wgs", "gemm_w4_diag_epi" (diagnostic builds), "adamw_blocks" (mm_adamw_step), and the "attn_*" switches of the attention
 * kernels.  A 0|1 switch stores value != 0; a value outside a switch's range returns MM_ERR_ARG and leaves the switch as it was;
 * unknown names return MM_ERR_ARG.                                                                                       */
int mm_set_option(const char* name, int value);
/* current value of a switch: every name mm_set_option answers (one table serves both; the "attn_*" names are answered by the
 * attention kernels' own pair of functions), so a caller that flips one temporarily can restore what it found.  MM_GEMM_KERNEL (environment, used while "gemm_kernel" is 0) does not show here.
 * Also the read-only "gemm_last_kernel": which kernel the last mm_gemm* / mm_decode_* call launched -- 0 the 128x128 register-staged
 * kernel (also the fallback past the 32-bit offsets), 1..5 the LDS-DMA tiles 256x128, 256x256 (8-wave), 128x128, 64x128, 64x64, 10
 * the 4-wave 256x256 kernel, 20 / 21 the M <= 16 weight-streaming kernels (gemm_skinny / gemv_stream: plain M <= 16 NT and the
 * decode fusions), 22 gemv_stream on MXFP8 weights (the mm_decode_*_w8 entry points), 23 the MXFP8 x MXFP8 scaled-MFMA kernel
 * (mm_gemm_mx8), 30 the fp32 kernel */
int mm_get_option(const char* name, int* value);
/* What a GEMM call with these facts would do, under the current switches: host only, launches nothing, needs no device when ncu
 * is given, and leaves "gemm_last_kernel" alone.  It is the function the launcher itself runs (csrc/mm_gemm_plan.h).
 * kind: 0 mm_gemm(_batched), 1 mm_gemm_act_fwd(_batched), 2 mm_gemm_swiglu_fwd (N = 2 swi_I), 3 mm_gemm_rope_fwd, 4 mm_gemm_swiglu_bwd
 * (N = I, K = H, ldaux = ldgu), after the entry point's own argument checks; groups: 0 = a stand-alone call; ptr_bits: the low four
 * address bits of A, B, C, bias, residual, aux (GU of swiglu_bwd), C2 (PRE / ACT) in nibbles 0..6 (a grouped call: OR-ed over its
 * problems); ncu: compute units, 0 = those of the current device.
 * plan[MM_GEMM_PLAN_INTS] receives: [0] the return code the call would give before launching, [1] "gemm_last_kernel" after the call
 * (-2: unchanged), [2] the kernel family (-1 none, 0 register-staged 128x128, 1 LDS-DMA, 2 4-wave, 3 gemm_skinny, 4 gemv_stream, 5
 * fp32), [3..10] its template arguments (register-staged {A_KC, B_KC}; LDS-DMA {A_KC, B_KC, BM, BN, WGM, STAGES, ISSUE_WAVES, EK};
 * 4-wave {A_KC, B_KC, EK, SCHED}; gemv_stream {MODE, NORM, NT}; fp32 {LAYOUT}; the rest 0), [11..14] grid x, grid y, block, dynamic
 * LDS bytes, [15..25] the kernel arguments nbm, nbn, tail, pipe, stagger, stagger_slots, diag_epi, shuffle, group_m, stream_epi,
 * rowmajor.  MM_ERR_ARG for a NULL plan or facts no entry point passes on (M, N <= 0, unknown layout / kind / epilogue bits).   */
enum { MM_GEMM_PLAN_INTS = 26 };
int mm_gemm_plan(int dtype, int layout, int kind, int groups, int M, int N, int K, int lda, int ldb, int ldc, int ldr, int ldaux,
                 int epilogue, int swi_I, int ptr_bits, int ncu, int* plan);

/* ---- GEMM: every nn.Linear / Conv2d(k=s) on the path -------------------------------------
 * replaces F.linear in mlp.py:33-39, HF:clip:280-384 (q/k/v/out/fc1/fc2), HF:clip:152-158 (patch conv as
 * GEMM), HF:llama:163-176,232-244,480 (gate/up/down, q/k/v/o, lm_head) and their autograd backward.
 * Requirements (MM_BF16): lda, ldb multiples of 8 elements and A, B 16-byte aligned; ldc (and ldr with MM_EPI_RESIDUAL)
 * multiples of 4 and C 8-byte aligned -- with ldc, ldr, N multiples of 8 and C, residual, bias 16-byte aligned the 256x256
 * kernel stores row-major 16-byte groups, otherwise 8-byte ones; for a K-contiguous operand whose K is not a multiple of 8
 * the row padding up to the next multiple of 8 must hold zeros (nothing beyond it is read).  Epilogue order, all in fp32
 * with ONE rounding to bf16 at the store: acc (+ bias) (activation) (+ residual) (+ C).                                  */
int mm_gemm(int dtype, int layout, int M, int N, int K, const void* A, int lda, const void* B, int ldb,
            void* C, int ldc, const void* bias, const void* residual, int ldr, int epilogue, void* stream);

/* Fused q|k|v projection + RoPE: qkv[M,N] = x[M,K] . W[N,K]^T (+ bias[N]) with the first rope_cols columns -- heads of width
 * head_dim = 128 -- rotated in the GEMM's epilogue by the per-token tables cos_t / sin_t [M, head_dim/2] f32 of mm_rope_table
 * (HF:llama:232-244 q/k/v_proj followed by apply_rotary_pos_emb :113-160); the remaining columns (v) are stored unrotated.
 * Bit-identical to mm_gemm + mm_rope_apply, one pass over q|k less.  MM_BF16; MM_ERR_UNSUPPORTED for other head widths, N or
 * rope_cols not multiples of 128, or M < 256 (use the two launches).                                                    */
int mm_gemm_rope_fwd(int dtype, int M, int N, int K, const void* X, int ldx, const void* W, int ldw, const void* bias, void* QKV,
                     int ldqkv, int rope_cols, int head_dim, const float* cos_t, const float* sin_t, void* stream);
/* SwiGLU MLP front half in ONE GEMM: replaces `act_fn(gate_proj(x)) * up_proj(x)` (HF:llama:163-176) = two F.linear + silu +
 * mul.  Wgu = the fused [2I, K] gate|up weight (gate rows first); GU [M, 2I] receives the bf16 pre-activations (what the two
 * linears would store; kept for backward), ACT [M, I] = bf16(bf16(silu(gate)) * up): bit-identical to mm_gemm + mm_swiglu_fwd.
 * bf16 only; MM_ERR_UNSUPPORTED when I % 128, K % 64 or M < 256 (use the two-launch form then).                              */
int mm_gemm_swiglu_fwd(int dtype, int M, int I, int K, const void* X, int ldx, const void* Wgu, int ldw, void* GU, int ldgu,
                       void* ACT, int ldact, void* stream);
/* Linear + GELU forward for TRAINING in one launch: ACT = act(X W^T + bias) (+ residual), PRE = the bf16 pre-activation
 * X W^T + bias that the activation's backward needs (CLIP MLP fc1, HF:clip:368-372; projector, mlp.py:33-39).  epilogue = exactly one
 * of MM_EPI_GELU_ERF / QUICK_GELU / GELU_TANH, optionally | MM_EPI_BIAS | MM_EPI_RESIDUAL.  Rounding points as in mm_gemm +
 * mm_gelu_fwd (+ mm_add): bit-identical.  bf16 only, M > 16 (MM_ERR_UNSUPPORTED otherwise: use the separate launches).          */
int mm_gemm_act_fwd(int dtype, int M, int N, int K, const void* X, int ldx, const void* W, int ldw, const void* bias,
                    void* PRE, int ldpre, void* ACT, int ldact, const void* residual, int ldr, int epilogue, void* stream);
/* backward of down_proj's input and of the SwiGLU in one launch: dGU [M, 2I] = swiglu'(GU) * (dY [M, H] . Wd [H, I]), the
 * product d(act) staying in registers (autograd of HF:llama:163-176; bit-identical to mm_gemm NN + mm_swiglu_bwd).          */
int mm_gemm_swiglu_bwd(int dtype, int M, int I, int H, const void* dY, int lddy, const void* Wd, int ldw, const void* GU,
                       int ldgu, void* dGU, int lddgu, void* stream);

/* column sums: out[N] (+)= sum_m X[m,n]   (bias gradients)                                           */
int mm_colsum(int dtype, const void* X, int M, int N, int ldx, void* out, int accumulate, void* stream);

/* ---- grouped launches: the expert as a batch dimension (MoE image modality: E CLIP towers of equal shape on every image;
 * reference modalities/image_modality_moe.py:150-161 loops the experts) ------------------------------------------------------
 * `groups` problems of EQUAL shape in one launch, 1 <= groups <= MM_GROUP_MAX (MM_ERR_ARG otherwise).  Per-problem pointers arrive as
 * HOST arrays of `groups` device pointers; the entry point copies them by value into the kernel's arguments: no device table, no
 * copy, no allocation, no synchronisation (capturable like the rest of the ABI).  Entries may repeat (the patch-embedding GEMM
 * reads the same patches for every expert) and need not be evenly spaced.  A NULL array or a NULL entry of a required operand is
 * MM_ERR_ARG.  All checks come before any launch.  Problem g's result has the bits the stand-alone entry point gives for it alone.
 * mm_gemm_batched: mm_gemm on every problem (alignment rules, epilogue order and the single rounding as there).  MM_F32, and for
 *   MM_BF16 the problems that take the 128x128, 64x128 or 64x64 tiles (chosen from the tile count of the WHOLE batch; every bf16
 *   kernel adds the products of a K-step in the same order, so the tile does not change the bits).  MM_ERR_UNSUPPORTED, before any
 *   launch, where mm_gemm would take a 256-wide tile, the M <= 16 weight-streaming kernels or an activation outside NT: those
 *   problems fill the chip on their own, so the caller loops mm_gemm (kernels.gemm_batched does).
 * mm_gemm_act_fwd_batched: mm_gemm_act_fwd (PRE and ACT per problem) under the same rules.  MM_ERR_UNSUPPORTED for MM_F32, for
 *   M <= 16 and under "gemm_kernel" = 1; ldpre a multiple of 4 and every PRE[g] 8-byte aligned (MM_ERR_ALIGN); N, K <= 0, a NULL PRE
 *   table or entry, no activation or more than one: MM_ERR_ARG.
 * mm_colsum_batched: mm_colsum per problem (the same row partition: same bits).
 * Alignment is that of the stand-alone entry point for EVERY problem: the low address bits are OR-ed over the problems, so one
 *   misaligned pointer in any problem is MM_ERR_ALIGN for the launch.  M == 0 or N == 0 (mm_gemm_batched), M == 0
 *   (mm_gemm_act_fwd_batched): MM_OK after the argument checks, nothing is launched or written.
 * "gemm_last_kernel": a grouped GEMM that launches sets it to the id of the tile the WHOLE batch ran on (3, 4, 5, or 30 for MM_F32);
 *   one that returns before launching -- any error code, or MM_OK for an empty problem -- leaves it as it was.
 * tests/test_grouped_contract_gpu.py holds these entry points to fp64 references, to the stand-alone bits and to these codes at
 *   the sizes where a workgroup walks several tiles and where the batch's tile differs from the stand-alone call's.          */
int mm_gemm_batched(int dtype, int layout, int groups, int M, int N, int K, const void* const* A, int lda, const void* const* B,
                    int ldb, void* const* C, int ldc, const void* const* bias, const void* const* residual, int ldr, int epilogue,
                    void* stream);
int mm_gemm_act_fwd_batched(int dtype, int groups, int M, int N, int K, const void* const* X, int ldx, const void* const* W, int ldw,
                            const void* const* bias, void* const* PRE, int ldpre, void* const* ACT, int ldact,
                            const void* const* residual, int ldr, int epilogue, void* stream);
int mm_colsum_batched(int dtype, const void* const* X, int groups, int M, int N, int ldx, void* const* out, int accumulate,
                      void* stream);

/* ids outside [0, vocab): *flag (device int, sticky) = 1.  nn.Embedding raises for them (model.py:433 embeds every id of the
 * batch before the splice); mm_embed_splice_fwd reads row 0 instead of out of bounds, so the caller checks this flag (the
 * Python layer reads it one call later, without a stall, and raises IndexError).  The flag is only ever set to 1: the
 * caller zeroes it, and a later call with good ids leaves a 1 in place.  T == 0: nothing is launched.                       */
int mm_embed_check_ids(const int64_t* ids, int T, int64_t vocab, int* flag, void* stream);

/* ---- embed + modality splice: model.py:433-444 ---------------------------------------------------
 * out[t,:] = proj[src[t],:] if src[t] >= 0 else emb[ids[t],:]; src is built from (batch_idx, token_range)
 * by mm_splice_build_map (last writer wins, like index_put).
 * Contract (tests/test_embed_contract_gpu.py):
 *   mm_splice_build_map writes all of src_map[0, T): -1, or the LARGEST source index i whose position
 *     pos(i) = batch_idx[i] * S + token_range[i] equals t.  A position outside [0, T) is dropped.  token_range is not
 *     checked against S: a value outside [0, S) lands in a neighbouring batch row (callers keep 0 <= token_range < S).
 *   mm_embed_splice_fwd copies rows bit for bit; an id outside [0, vocab) reads row 0 (see mm_embed_check_ids).  H % vn == 0
 *     (vn = 8 bf16, 4 fp32) and emb, proj, out 16-byte aligned, else MM_ERR_ALIGN; a src_map without proj is MM_ERR_ARG.
 *     Every row of out is written exactly once and nothing behind row T - 1.                            */
int mm_splice_build_map(const int64_t* batch_idx, const int64_t* token_range, int n_mod, int S, int T,
                        int32_t* src_map, void* stream);
int mm_embed_splice_fwd(int dtype, const void* emb, int64_t vocab, int H, const int64_t* ids, const void* proj,
                        const int32_t* src_map, int T, void* out, void* stream);
/* token order for the embedding gradient (depends on ids / src_map only, so it is built at forward time): a stable
 * sort of the T tokens by id; tokens overwritten by a modality row or with an id outside [0, vocab) sort last and get no
 * gradient.  order/skey: int32 [order_elems]; key_ws: int32 [T] workspace; sizes from mm_embed_sort_sizes.
 * Contract: order[0, T) = the stable sort of the tokens by (key, t), key = id or 0x7fffffff for a token that gets no gradient;
 * order[T, order_elems) is NOT written (and never read for a token); skey[0, order_elems) = the sorted keys followed by
 * 0x7fffffff, order_elems = (ceil(T / 32) + 1) * 32.  The same permutation on every launch.                            */
int mm_embed_sort_sizes(int T, int H, int64_t* order_elems, int64_t* scratch_floats);
int mm_embed_sort(const int64_t* ids, const int32_t* src_map, int T, int64_t vocab, int32_t* key_ws, int32_t* order,
                  int32_t* skey, void* stream);
/* backward (autograd of model.py:433-444): dproj[i,:] = dE[pos(i),:]; demb[id,:] (+)= sum of dE[t,:] over the tokens t
 * with ids[t] == id that were NOT overwritten -- summed in fp32 in ascending token order, rounded once, one write per
 * touched row: bitwise reproducible, no atomics.  accumulate = 0 overwrites the touched rows (the caller has zeroed
 * demb), 1 adds to what demb holds (tied lm_head gradient, gradient accumulation).  scratch: fp32 [scratch_floats].
 * Contract: a row of demb that no valid token touches keeps its bits in both modes.  A row's sum takes at most 32 adds inside
 * a chunk of 32 sorted positions plus one per further chunk its run spans; its value does not depend on what scratch held (two
 * slots per chunk, each read only after this call wrote it).  dproj[i] is a bit copy of dE[pos(i)] for the source that owns its
 * position and exactly zero for a lost duplicate or a dropped position; dproj needs batch_idx, token_range and src_map, demb
 * needs ids, order, skey and scratch (MM_ERR_ARG).  H % vn == 0, dE, demb and scratch 16-byte aligned (MM_ERR_ALIGN).       */
int mm_embed_splice_bwd(int dtype, const void* dE, int H, const int64_t* ids, const int32_t* src_map, int T,
                        const int64_t* batch_idx, const int64_t* token_range, int n_mod, int S, void* dproj,
                        void* demb, int64_t vocab, const int32_t* order, const int32_t* skey, float* scratch,
                        int accumulate, void* stream);

/* ---- ViT patch embedding glue: HF:clip:138-218 -----------------------------------------------------
 * patchify: pixels f32 [n,3,Himg,Wimg] -> patches [n*P, Kpad] (k = c*ps*ps + py*ps + px, zero padded)
 * P = (Himg / ps) * (Wimg / ps), patch (row r, column q) of the grid in row r * (Wimg / ps) + q; each element is the pixel rounded
 * once to the dtype, columns [3 ps^2, Kpad) are exactly zero, a ragged border (Himg % ps rows, Wimg % ps columns) is dropped.  */
int mm_patchify(int dtype, const float* pixels, int n, int himg, int wimg, int ps, int kpad, void* patches, void* stream);
/* x[n,0,:] = cls + pos[0]; x[n,1+p,:] = patch_out[n*P+p,:] + pos[1+p]: one fp32 add rounded once (no alignment rule)  */
int mm_vit_embed_fwd(int dtype, const void* patch_out, const void* cls, const void* pos, int n, int P, int D,
                     void* x, void* stream);
/* dpatch_out = dx[:,1:,:] (bit copy); dcls (+)= sum_n dx[n,0]; dpos (+)= sum_n dx[n]: the fp32 sum over the images in
 * index order, + the old value when accumulate, rounded once.  Each of the three outputs may be NULL (skipped); without
 * accumulate the old contents of dcls / dpos are not read.                                                 */
int mm_vit_embed_bwd(int dtype, const void* dx, int n, int P, int D, void* dpatch_out, void* dcls, void* dpos,
                     int accumulate, void* stream);
/* dst[n,P,D] = src[n,1+P,D][:,1:,:] (image_modality.py:133) and its adjoint (zero CLS row)                */
/* ---- plug-in towers without a CLS token and with head_dim outside {64,128} (SigLIP-so400m: 16 heads x 72) ----------
 * mm_bcast_add: y[n,L] = x[n,L] + b[L]  (learned positions added to every image; HF:siglip SiglipVisionEmbeddings)
 * mm_head_pad:  inverse = 0: dst[rows, nheads*dpad] = src[rows, nheads*d] with each head zero-padded to dpad;
 *               inverse = 1: dst[rows, nheads*d] = the first d columns of every head of src[rows, nheads*dpad].
 *               Zero columns change neither q.k nor p.v, so attention on the padded heads is exact.
 * Contract of the movers (bcast_add, head_pad, drop_cls, rows_select): rows are bit copies, mm_bcast_add is one fp32 add rounded
 * once; widths (L, d, dpad, D, ld_src, ld_dst) % vn == 0 and every pointer 16-byte aligned, else MM_ERR_ALIGN; dpad < d is
 * MM_ERR_ARG, a dtype other than MM_BF16 / MM_F32 is MM_ERR_UNSUPPORTED for bcast_add and head_pad.  mm_head_pad writes the
 * whole padded head (zeros in [d, dpad)); its inverse does not read the pad.  mm_rows_select writes dst[r, 0:D) only (columns
 * [D, ld_dst) stay untouched, ld < D is MM_ERR_ALIGN).  An empty call (n, rows or n_dst == 0) launches nothing.            */
int mm_bcast_add(int dtype, const void* x, const void* b, int n, int64_t L, void* y, void* stream);
int mm_head_pad(int dtype, const void* src, int64_t rows, int nheads, int d, int dpad, void* dst, int inverse, void* stream);
int mm_drop_cls_fwd(int dtype, const void* src, int n, int P, int D, void* dst, void* stream);
int mm_drop_cls_bwd(int dtype, const void* ddst, int n, int P, int D, void* dsrc, void* stream);
/* Loss rows (HF:loss/loss_utils.py:36-71 ignores labels == -100; llama modeling's lm_head + loss_function call): the training
 * step computes the final norm, lm_head and the loss only on the rows that carry a label.  dst[r, :D] = src[map[r], :D], or
 * zeros where map[r] < 0 (or >= n_src).  Forward: map = indices of the labelled rows; backward: map = the inverse map.       */
int mm_rows_select(int dtype, const void* src, int64_t ld_src, const int* map, int n_src, int n_dst, int D, void* dst,
                   int64_t ld_dst, void* stream);

/* ---- norms ------------------------------------------------------------------------------------------
 * Widths (all four norm entries): H % 8 == 0 for MM_BF16, H % 4 == 0 for MM_F32 (MM_ERR_ALIGN otherwise), and a row of at most
 * 256 * 8 sixteen-byte vectors: H <= 16384 for MM_BF16, H <= 8192 for MM_F32 (MM_ERR_UNSUPPORTED above).  M == 0 writes nothing.
 * RMSNorm: HF:llama:53-70.  rstd[M] f32 is saved for backward.  Rounding points (T = the storage type): fp32 sum of squares (any
 * order), rstd = rsqrtf(ss / H + eps), y = T(w * f32(T(x * rstd))): the normalised value is rounded to T BEFORE the weight
 * multiply, as HF's `weight * hidden_states.to(input_dtype)`.  Given the kernel's own rstd, y is bit-identical to that chain.   */
int mm_rmsnorm_fwd(int dtype, const void* x, const void* w, int M, int H, float eps, void* y, float* rstd, void* stream);
/* dx = rstd*(g - xhat*mean(g*xhat)) (+ dres), g = dy*w;  dw_partial[nblk,H] f32 (nblk = mm_norm_bwd_blocks(M)).
 * dres (optional, [M,H]) is the gradient arriving through the residual branch that shares x: fusing the add here
 * replaces autograd's separate accumulation pass.                                                              */
int mm_rmsnorm_bwd(int dtype, const void* dy, const void* x, const void* w, const float* rstd, int M, int H,
                   void* dx, float* dw_partial, const void* dres, void* stream);
/* LayerNorm: HF:clip:338-339,608 (nn.LayerNorm).  mean/rstd [M] f32 saved.                                 */
int mm_layernorm_fwd(int dtype, const void* x, const void* w, const void* b, int M, int H, float eps, void* y,
                     float* mean, float* rstd, void* stream);
int mm_layernorm_bwd(int dtype, const void* dy, const void* x, const void* w, const float* mean, const float* rstd,
                     int M, int H, void* dx, float* dw_partial, float* db_partial, const void* dres, void* stream);
int mm_norm_bwd_blocks(int M);
/* out[H] (+)= sum_b partial[b,H]  (f32 partials -> param-dtype gradient)                                    */
int mm_reduce_partials(int dtype, const float* partial, int nblk, int H, void* out, int accumulate, void* stream);
/* the same for two (partials, output) pairs in one launch: LayerNorm's dw and db */
int mm_reduce_partials2(int dtype, const float* partial0, const float* partial1, int nblk, int H, void* out0, void* out1, int accumulate0,
                        int accumulate1, void* stream);
/* Grouped LayerNorm (conventions of mm_gemm_batched): x, y, dy, dx, dres are ONE expert-major buffer [groups * R, H], mean / rstd
 * [groups * R]; w[] / b[] are per expert.  A backward workgroup never spans two experts: expert g owns the partial blocks
 * [g * nb, (g + 1) * nb), nb = mm_norm_bwd_blocks(R), partitioned as a stand-alone call with M = R partitions them (dw_partial /
 * db_partial: f32 [groups * nb, H]).  mm_reduce_partials2_batched reduces expert g's nblk blocks into out0[g] / out1[g] in the
 * order of mm_reduce_partials2.  Every output has the bits of `groups` stand-alone calls.  Widths as for the stand-alone norms
 * (MM_ERR_ALIGN / MM_ERR_UNSUPPORTED), checked before any launch; R == 0: MM_OK, nothing is launched or written; nblk == 0: out0[g] /
 * out1[g] = 0, or stay under their `accumulate`.  groups outside 1..MM_GROUP_MAX, a NULL table or a NULL entry: MM_ERR_ARG.          */
int mm_layernorm_fwd_batched(int dtype, const void* x, const void* const* w, const void* const* b, int groups, int R, int H, float eps,
                             void* y, float* mean, float* rstd, void* stream);
int mm_layernorm_bwd_batched(int dtype, const void* dy, const void* x, const void* const* w, int groups, const float* mean,
                             const float* rstd, int R, int H, void* dx, float* dw_partial, float* db_partial, const void* dres,
                             void* stream);
int mm_reduce_partials2_batched(int dtype, const float* partial0, const float* partial1, int groups, int nblk, int H, void* const* out0,
                                void* const* out1, int accumulate0, int accumulate1, void* stream);

/* ---- RoPE: HF:llama:113-160 (rotate_half form) --------------------------------------------------------
 * cos/sin tables [T, D/2] f32 from position_ids and inv_freq (HF:llama:113-127; llama3 scaling is applied by
 * the caller to inv_freq, HF:modeling_rope_utils.py:641-662).  round_bf16: round cos/sin to bf16 (HF casts them
 * to the activation dtype).  The angle is ONE fp32 product float(position) * inv_freq[j] (HF's fp32 matmul of a single term);
 * the tables are cosf / sinf of that fp32 angle, so they follow the angle's rounding at large positions, as HF's do.           */
int mm_rope_table(const int64_t* position_ids, const float* inv_freq, int T, int half, int round_bf16, float* cos_t,
                  float* sin_t, void* stream);
/* in place on x viewed as [T, nheads, D] with row stride ld (elements); inverse=1 applies the adjoint          */
int mm_rope_apply(int dtype, void* x, int T, int nheads, int D, int ld, const float* cos_t, const float* sin_t,
                  int inverse, void* stream);

/* ---- attention: HF:llama:191-213 (eager softmax attention, GQA via repeat_kv), HF:clip:280-334 ------------
 * q [B,Sq,Hq,D], k/v [B,Skv,Hkv,D] with element strides (batch, seq, head); D contiguous; D in {64,128} for
 * MM_BF16 (MFMA path), any D<=256 for MM_F32.  key_mask [B,Skv] int64 (1 = attend) or NULL.  causal aligns the
 * LAST query with the LAST key (q position = i + Skv - Sq).  out [B,Sq,Hq,D] contiguous; lse [B,Hq,Sq] f32.
 * Sq > Skv is allowed: under causal the first Sq - Skv queries then see no key.  A query row with no visible key (causal
 * and/or key_mask) gives out = 0 and lse = +inf, never NaN, and dq = 0 in mm_attn_bwd; a key no query sees gets dk = dv = 0.
 * Known limit of the MM_BF16 D = 128 kernels: a buffer resource spans at most 4 GiB of one head's K or V rows
 * ((Skv - 1) * k_ss * 2 bytes), about 349 k keys in the Llama fused qkv layout.                                 */
int mm_attn_fwd(int dtype, const void* q, const void* k, const void* v, int B, int Sq, int Skv, int Hq, int Hkv, int D,
                int64_t q_sb, int64_t q_ss, int64_t q_sh, int64_t k_sb, int64_t k_ss, int64_t k_sh, int64_t v_sb,
                int64_t v_ss, int64_t v_sh, const int64_t* key_mask, int causal, float scale, void* out, float* lse,
                void* stream);
/* dq/dk/dv use the SAME strides as q/k/v.  delta [B,Hq,Sq] f32 workspace.  dk/dv are overwritten.
 * For MM_F32 dk/dv must be zero-filled by the caller (atomic accumulation).                                   */
int mm_attn_bwd(int dtype, const void* q, const void* k, const void* v, const void* out, const void* dout, const float* lse,
                int B, int Sq, int Skv, int Hq, int Hkv, int D, int64_t q_sb, int64_t q_ss, int64_t q_sh, int64_t k_sb,
                int64_t k_ss, int64_t k_sh, int64_t v_sb, int64_t v_ss, int64_t v_sh, const int64_t* key_mask, int causal,
                float scale, void* dq, void* dk, void* dv, float* delta, void* stream);

/* Decode step: mm_rope_apply on the q and k heads of x [T, (Hq+2Hkv)*D] (row stride ld) plus, in the same pass, the append
 * of the roped k heads and the v heads to the KV cache (HF cache update inside LlamaAttention.forward, HF:llama:247-252):
 * kdst / vdst point at the cache row of this step for sequence 0 ([Hkv, D] contiguous), dstride = elements between
 * consecutive sequences' rows (one token per sequence: T = batch).                                                   */
int mm_rope_append(int dtype, void* x, int T, int Hq, int Hkv, int D, int ld, const float* cos_t, const float* sin_t,
                   void* kdst, void* vdst, int64_t dstride, void* stream);

/* ---- Qwen3 per-head q/k RMSNorm + RoPE (HF 5.15 models/qwen3/modeling_qwen3.py:50-64,237-257):
 * q = RoPE(q_norm(q_proj(h).view(.., Hq, D))), k = RoPE(k_norm(k_proj(h).view(.., Hkv, D))), w_q / w_k [D].  bf16 or f32; D in
 * {64, 128} (MM_ERR_UNSUPPORTED otherwise).  cos_t / sin_t: mm_rope_table's [T, D/2] tables.
 * mm_qk_norm_rope_fwd: x = the q|k heads [T, (Hq+Hkv)*D] (row stride ld_in; the q|k columns of the fused projection output)
 *   -> out [T, (Hq+Hkv)*D] (row stride ld_out) and rstd [T, Hq+Hkv] f32 (may be NULL).  Per head: fp32 sum of squares (any order),
 *   rstd = rsqrtf(ss/D + eps), y = bf16(w * bf16(x*rstd)) (mm_rmsnorm_fwd's rounding points), then mm_rope_apply's rotation of y:
 *   given the kernel's own rstd, out is bit-identical to that chain followed by mm_rope_apply.  out == x (with ld_out == ld_in)
 *   runs in place: every lane stores only the elements it loaded.
 * mm_qk_norm_rope_bwd: dqk = d(out) (row stride ld_dqk), x / rstd as in forward -> dx (row stride ld_dx; the q|k columns of the
 *   projection's dqkv, nothing else is written): inverse RoPE, then mm_rmsnorm_bwd's dx = rstd*(g - xhat*mean(g*xhat)), g = dy*w.
 *   dwq_partial / dwk_partial [mm_qk_norm_bwd_blocks(T), D] f32 (reduce with mm_reduce_partials): deterministic, no atomics;
 *   both NULL skips dw (frozen norms; dx is still written).
 * mm_qk_norm_rope_append: decode step: the forward in place on the q|k heads of x [T, (Hq+2Hkv)*D] (row stride ld) plus the append
 *   of the normed, roped k heads and the v heads to the KV cache rows kdst / vdst, as mm_rope_append.  Same head code as the forward:
 *   bit-identical to mm_qk_norm_rope_fwd in place followed by the cache copy.                                                   */
int mm_qk_norm_rope_fwd(int dtype, const void* x, int ld_in, int T, int Hq, int Hkv, int D, const void* w_q, const void* w_k, float eps,
                        const float* cos_t, const float* sin_t, void* out, int ld_out, float* rstd, void* stream);
int mm_qk_norm_bwd_blocks(int T);
int mm_qk_norm_rope_bwd(int dtype, const void* dqk, int ld_dqk, const void* x, int ld_x, int T, int Hq, int Hkv, int D, const void* w_q,
                        const void* w_k, const float* rstd, const float* cos_t, const float* sin_t, void* dx, int ld_dx, float* dwq_partial,
                        float* dwk_partial, void* stream);
int mm_qk_norm_rope_append(int dtype, void* x, int T, int Hq, int Hkv, int D, int ld, const void* w_q, const void* w_k, float eps,
                           const float* cos_t, const float* sin_t, void* kdst, void* vdst, int64_t dstride, void* stream);

/* ---- decode-step fusions on the weight-streaming GEMM (KV-cache decode of `generate`, reference model.py:595-602; M = batch <= 16;
 * MM_BF16).  Each replaces a GEMM + the tiny launches around it in HF's LlamaDecoderLayer (HF:llama:284-325) with the arithmetic
 * and rounding points of the separate kernels (same bits).  `in_norm_w` (may be NULL) / `eps`: the RMSNorm IN FRONT of the projection
 * (input_layernorm, post_attention_layernorm, the model's final norm), applied to x while it is staged: y = x' W^T with
 * x' = RMSNorm(x) * in_norm_w.  M * K * 2 bytes of x must fit 144 KB of LDS (MM_ERR_UNSUPPORTED otherwise: use the separate kernels).
 * mm_decode_gateup_swiglu:   ACT[M,I] = silu(x' Wg^T) * (x' Wu^T), Wgu = fused [2I,K] gate|up weight    (= [mm_rmsnorm_fwd +] mm_gemm + mm_swiglu_fwd)
 * mm_decode_qkv_rope_append: QKV[M,(Hq+2Hkv)*128] = x' W^T (+ bias), q and k heads rotated with cos_t / sin_t [M,64], roped k and v
 *                            appended to the KV cache rows kdst / vdst (+ m * dstride)                  (= [mm_rmsnorm_fwd +] mm_gemm + mm_rope_append)
 * mm_decode_linear:          C[M,N] = x' W^T (+ bias) (+ residual)                                      (= [mm_rmsnorm_fwd +] mm_gemm)             */
int mm_decode_gateup_swiglu(int dtype, int M, int I, int K, const void* X, int ldx, const void* Wgu, int ldw, void* ACT, int ldact,
                            const void* in_norm_w, float eps, void* stream);
int mm_decode_qkv_rope_append(int dtype, int M, int Hq, int Hkv, int D, int K, const void* X, int ldx, const void* W, int ldw,
                              const void* bias, void* QKV, int ldqkv, const float* cos_t, const float* sin_t, void* kdst, void* vdst,
                              int64_t dstride, const void* in_norm_w, float eps, void* stream);
int mm_decode_linear(int dtype, int M, int N, int K, const void* X, int ldx, const void* W, int ldw, const void* bias,
                     const void* residual, int ldr, void* C, int ldc, const void* in_norm_w, float eps, void* stream);

/* ---- weight-only MXFP8 for the decode step (opt-in).  A row-major bf16 matrix W[N,K], K % 32 == 0, is stored as OCP e4m3fn elements
 * with one power-of-two scale byte (E8M0: 2^(byte - 127)) per block of 32 consecutive k of a row: 1 + 1/32 byte per weight.
 * Per block: amax = largest |w|; e = the SMALLEST integer with amax * 2^-e <= 448, i.e. e0 = floor(log2 amax) - 8, or e0 + 1 when
 * amax * 2^-e0 > 448 (the OCP "floor" rule would saturate the block's largest element there); scale byte = clamp(e + 127, 27, 254),
 * 127 for an all-zero block; element = e4m3fn(clamp(w * 2^-e, -448, 448)), round to nearest even, sign of zero kept.  The lower
 * clamp keeps every dequantised value a normal bf16, and an e4m3 value times a power of two IS a bf16 number: the dequantised matrix W'
 * is an ordinary bf16 tensor, exactly.  NaN / Inf in W are outside the contract (the result is unspecified).
 * The layout of the packed buffer is private to the library (csrc/mm_mxfp8.h) and depends on (N, K) only.
 * mm_mxfp8_bytes:   bytes of the packed buffer of W[N,K] (elements + scales, a multiple of 16); negative (MM_ERR_UNSUPPORTED) if K % 32.
 * mm_quant_mxfp8:   W (row stride ldw >= K elements, ldw % 8 == 0, 16-byte aligned) -> packed (16-byte aligned, mm_mxfp8_bytes); one pass.
 * mm_dequant_mxfp8: packed -> Wd = W' (bf16, row stride ldd).
 * mm_decode_*_w8:   the three decode fusions above with `packed` in place of (W, ldw) -- for mm_decode_gateup_swiglu_w8 the fused
 *                   [2I,K] gate|up matrix quantised as one matrix.  Bit-identical to the bf16 entry point run on W' (every MFMA sees
 *                   the same K elements).  MM_ERR_UNSUPPORTED before any launch if K % 32 or x does not fit the LDS stage.         */
int64_t mm_mxfp8_bytes(int N, int K);
int mm_quant_mxfp8(const void* W, int ldw, int N, int K, void* packed, void* stream);
int mm_dequant_mxfp8(const void* packed, int N, int K, void* Wd, int ldd, void* stream);
int mm_decode_gateup_swiglu_w8(int dtype, int M, int I, int K, const void* X, int ldx, const void* packed, void* ACT, int ldact,
                               const void* in_norm_w, float eps, void* stream);
int mm_decode_qkv_rope_append_w8(int dtype, int M, int Hq, int Hkv, int D, int K, const void* X, int ldx, const void* packed,
                                 const void* bias, void* QKV, int ldqkv, const float* cos_t, const float* sin_t, void* kdst, void* vdst,
                                 int64_t dstride, const void* in_norm_w, float eps, void* stream);
int mm_decode_linear_w8(int dtype, int M, int N, int K, const void* X, int ldx, const void* packed, const void* bias,
                        const void* residual, int ldr, void* C, int ldc, const void* in_norm_w, float eps, void* stream);

/* ---- MXFP8 x MXFP8 GEMM for the prefill (opt-in), on gfx950's block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4, e4m3 both sides).
 * packedW: the buffer mm_quant_mxfp8 writes for W[N,K], byte for byte (the decode step's copy: no second one); packedA: the same
 * format for the activation rows, mm_quant_mxfp8(X, ldx, M, K, ...).  Both 16-byte aligned and of mm_mxfp8_bytes; nothing past them
 * is read.
 *   C[m,n] = bf16( sum_k A'[m,k] W'[n,k] (+ bias[n]) (+ residual[m,n]) ),   A', W' = mm_dequant_mxfp8 of the two buffers,
 * bf16 C (row stride ldc >= N), bias, residual (row stride ldr >= N); fp32 accumulation in a fixed order (no atomics, no split-K: the
 * same call gives the same bits), bias then residual added in fp32, ONE rounding at the store.  residual may be C itself.  No alignment
 * rule on C / residual / ldc beyond the bf16 element (8-byte groups are stored where the address allows).
 * epi: MM_EPI_BIAS | MM_EPI_RESIDUAL only (MM_ERR_UNSUPPORTED for any other bit).  M, N >= 1 with row / column tails inside a tile;
 * K % 128 == 0 and K <= 2^20, else MM_ERR_UNSUPPORTED (every such width is taken; the ones whose layout carries padding slots --
 * 3584, 18944, ... -- walk the padding as zeros).  M, N, K <= 0, a NULL operand, ldc / ldr < N: MM_ERR_ARG; a misaligned buffer:
 * MM_ERR_ALIGN.  All checks come before the launch; a refused call writes nothing.  "gemm_last_kernel" reads 23 after a launch.
 * mm_gemm_mx8_supported: 0, or the MM_ERR_* the shape alone would get from mm_gemm_mx8; host only, launches nothing, needs no device. */
int mm_gemm_mx8(int M, int N, int K, const void* packedA, const void* packedW, const void* bias, const void* residual, int ldr,
                void* C, int ldc, int epi, void* stream);
int mm_gemm_mx8_supported(int M, int N, int K);

/* KV-cache decode step: ONE query token per sequence over the cached keys (reference model.py:595-602 calling the LLM with
 * past_key_values; HF:llama:217-281 with q_len = 1).  q [B,Hq,D] (strides q_sb,q_sh; D contiguous), k/v [B,Skv,Hkv,D] as
 * in mm_attn_fwd, key_mask [B,Skv] or NULL, out [B,Hq,D] contiguous.  MM_BF16, D in {64,128}, Hq/Hkv in {1,2,4,7,8}.
 * workspace: f32 [B*Hq*nsplit*(D+2)] with nsplit = mm_attn_decode_splits(B,Hkv,Skv) (slices of the keys, merged in a
 * fixed order).  sync: int [B*Hkv], zero on entry and left zero -- the slice that arrives last does the merge inside
 * the same launch; NULL = merge in a second launch.  Rows with no visible key give 0.
 * Any nsplit >= 1 is accepted (the workspace is sized by the nsplit passed): slice s holds keys [s*chunk, min(Skv, (s+1)*chunk))
 * with chunk = ceil(Skv / nsplit), and a slice with no key or with masked keys only adds nothing.  Masked keys (key_mask = 0
 * inside [0, Skv)) must hold finite values: the MFMA slice kernel forms 0 * v for them; rows from Skv on are never read.
 * MM_ERR_ARG: Hq % Hkv != 0, nsplit < 1, Skv <= 0, a NULL operand; MM_ERR_UNSUPPORTED: another dtype, D or Hq/Hkv;
 * MM_ERR_ALIGN: a stride that is not a multiple of 8 elements, q / k / v not 16-byte aligned; B = 0: MM_OK, nothing written.  */
int mm_attn_decode_splits(int B, int Hkv, int Skv);
int mm_attn_decode(int dtype, const void* q, const void* k, const void* v, int B, int Skv, int Hq, int Hkv, int D,
                   int64_t q_sb, int64_t q_sh, int64_t k_sb, int64_t k_ss, int64_t k_sh, int64_t v_sb, int64_t v_ss,
                   int64_t v_sh, const int64_t* key_mask, float scale, void* out, float* workspace, int nsplit, int* sync,
                   void* stream);

/* Decode step of n samples per prompt over ONE copy of the prompt's keys (generate's num_return_sequences; opt-in).  Query row
 * r = b*n + j of q [B*n,Hq,D] (strides q_sb,q_sh) is sample j of prompt b; it attends over Skv = Sp + Ss keys: prompt b's prefix
 * kp/vp [B,Sp,Hkv,D] followed by row r's own suffix ks/vs [B*n,Ss,Hkv,D] (element strides as in mm_attn_decode), one softmax over the
 * concatenation.  key_mask [B,Sp] or NULL applies to the prefix; suffix keys are always visible.  out [B*n,Hq,D] contiguous.
 * MM_BF16, D = 128, Hq/Hkv = G in {1,2,4}, any n >= 1: the kernel packs 16/G samples per 16-column MFMA tile (the columns
 * mm_attn_decode's MFMA slice kernel pads with zeros), so a prefix key is read once per tile, not once per sample; further samples
 * take further tiles (workgroups).  Anything else is MM_ERR_UNSUPPORTED.
 * Slices are mm_attn_decode's over the concatenation: chunk = ceil(Skv / nsplit), slice s holds keys [s*chunk, min(Skv, (s+1)*chunk))
 * -- in the prefix, across Sp, in the suffix, or empty; every slice writes its record.  workspace: f32 [B*n*Hq*nsplit*(D+2)] in
 * mm_attn_decode's record format, merged by the same second launch (there is no single-launch form).  Any nsplit >= 1 is accepted.
 * Bit identity: for every accepted shape and nsplit, out has the bits of mm_attn_decode (sync = NULL, "attn_decode_mfma" = 1) run with
 * the same nsplit on the materialised k/v [B*n,Sp+Ss,Hkv,D] and mask cat(mask.repeat_interleave(n,0), ones): a score is one MFMA
 * output element, which does not depend on the other columns, and the softmax, the P.V chain and the merges keep that kernel's order.
 * Masked prefix keys must hold finite values; rows of either cache beyond Sp / Ss are never read and nothing stored there matters.
 * MM_ERR_ARG: a NULL operand, Sp < 1, Ss < 1, n < 1, nsplit < 1, Hq % Hkv != 0, more than 65535 (prompt, tile) pairs; MM_ERR_ALIGN: a
 * stride that is not a multiple of 8 elements, q / kp / vp / ks / vs not 16-byte aligned.  Every check comes before any launch;
 * B = 0: MM_OK, nothing written.
 * mm_attn_decode_shared_splits: the slice count from the "attn_decode_wgs" workgroup target of mm_attn_decode_splits, at least 64
 * keys per slice: ceil(T / (B * ceil(n/4) * Hkv)) with T = ceil(2 * attn_decode_wgs / 3).  The workgroups counted are this launch's
 * at G = 4, the most an accepted shape launches (G is not an argument; G < 4 launches fewer, never more).  Two thirds: the option
 * stands for ~3 workgroups per CU of mm_attn_decode's slice kernel, and this kernel's 16 columns of accumulators let a CU hold two
 * (measured: profiles/r08_shared_prefix.md).  1 when the option is 1.                                                            */
int mm_attn_decode_shared_splits(int B, int n, int Hkv, int Skv);
int mm_attn_decode_shared(int dtype, const void* q, const void* kp, const void* vp, const void* ks, const void* vs, int B, int n,
                          int Sp, int Ss, int Hq, int Hkv, int D, int64_t q_sb, int64_t q_sh, int64_t kp_sb, int64_t kp_ss,
                          int64_t kp_sh, int64_t vp_sb, int64_t vp_ss, int64_t vp_sh, int64_t ks_sb, int64_t ks_ss, int64_t ks_sh,
                          int64_t vs_sb, int64_t vs_ss, int64_t vs_sh, const int64_t* key_mask, float scale, void* out,
                          float* workspace, int nsplit, void* stream);

/* mm_attn_decode_beam (generate's num_beams; opt-in): mm_attn_decode_shared with an ancestor table anc, int32 [Ss, anc_ld] with
 * anc_ld >= B*n.  Query row r of prompt b attends over [prefix of b | suffix key t read from PHYSICAL suffix row anc[t*anc_ld + r],
 * t < Ss]: a beam continues another row's generated suffix without a copy of the cache.  The kernel clamps every entry it reads into
 * its own prompt's rows [b*n, b*n + n), so no table can make it read outside ks / vs.  Slices, workspace, the merge launch, the
 * accepted shapes and every refusal are mm_attn_decode_shared's; a NULL anc or anc_ld < B*n is MM_ERR_ARG.
 * Bit identity: the table anc[t][r] = r gives mm_attn_decode_shared's bits, and any table with entries in range gives the bits of
 * mm_attn_decode_shared on the gathered suffix ks'[r, t] = ks[anc[t][r], t] (vs alike): only the row address of a suffix key
 * changes.  mm_attn_decode_shared itself is the kernel it was (the table is a template argument of the kernel, not a branch). */
int mm_attn_decode_beam(int dtype, const void* q, const void* kp, const void* vp, const void* ks, const void* vs, int B, int n,
                        int Sp, int Ss, int Hq, int Hkv, int D, int64_t q_sb, int64_t q_sh, int64_t kp_sb, int64_t kp_ss,
                        int64_t kp_sh, int64_t vp_sb, int64_t vp_ss, int64_t vp_sh, int64_t ks_sb, int64_t ks_ss, int64_t ks_sh,
                        int64_t vs_sb, int64_t vs_ss, int64_t vs_sh, const int64_t* key_mask, float scale, void* out,
                        float* workspace, int nsplit, const int32_t* anc, int anc_ld, void* stream);

/* mm_attn_decode_verify (generate's prompt_lookup_num_tokens; opt-in): Q causal query positions per sequence over ONE read of the
 * sequence's keys, with per-sequence lengths that live on the device.  q [B*Q,Hq,D] (strides q_sb per row, q_sh; row b*Q + j is
 * position j of sequence b), k/v [B,Scap,Hkv,D] a view of the cache (element strides as in mm_attn_decode), key_mask [B,Sp] or NULL
 * over the prompt (0 <= Sp <= Scap; ignored when key_mask is NULL), base int32 [B] on the device, out [B*Q,Hq,D] contiguous.
 * Query (b, j) sees key t iff t <= base[b] + j and (t >= Sp or key_mask[b,t] != 0).  The kernel clamps base[b] into [0, Scap - Q], so
 * no value can make it read outside the view.  MM_BF16, D = 128, Hq/Hkv = G in {1,2,4}, 1 <= Q <= 16, Scap >= Q; another dtype, D
 * or G is MM_ERR_UNSUPPORTED.  A 16-column MFMA tile packs 16/G query positions of one sequence (column jl*G + g is head g
 * of the tile's position jl), so a key is read once per tile; further positions take further tiles (workgroups).
 * Slices, workspace, merge: mm_attn_decode_shared's.  Slices cover [0, Scap) -- a bound the host knows without a sync -- with chunk =
 * ceil(Scap / nsplit); slice s holds keys [s*chunk, min(Scap, (s+1)*chunk)); a slice past a row's length writes a neutral record
 * (m = -inf, l = 0, o = 0).  workspace: f32 [B*Q*Hq*nsplit*(D+2)] in mm_attn_decode's record format, merged by the same second
 * launch.  Any nsplit >= 1 is accepted.  Keys in [0, base[b] + Q) (after the clamp) are read and must be finite, masked ones
 * included; rows from base[b] + Q on are never read and nothing stored there matters.  A row with no visible key gives 0.
 * Bit identity: for every accepted shape and nsplit, out[b*Q + j] has the bits of mm_attn_decode (sync = NULL, "attn_decode_mfma" = 1,
 * the same nsplit) run on ONE row: q[b*Q + j] over k/v[b, :Scap] (finite everywhere) with the mask [key_mask[b] | ones up to
 * base[b] + j | zeros after]: a score is one MFMA output element, which does not depend on the other columns; a key the mask hides
 * contributes p = 0 exactly, whatever finite value stands in its place; the softmax, the P.V chain and the merges keep that kernel's
 * order.
 * MM_ERR_ARG: a NULL operand (q, k, v, base, out, workspace), B < 0, Q outside [1, 16], Scap < Q, Sp outside [0, Scap] with a mask,
 * nsplit < 1, Hq % Hkv != 0, more than 65535 (sequence, tile) pairs; MM_ERR_ALIGN: a stride that is not a multiple of 8 elements, q / k
 * / v not 16-byte aligned.  Every check comes before any launch; B = 0: MM_OK, nothing written.  No allocation, copy or
 * synchronisation inside (capturable).
 * mm_attn_decode_verify_splits: mm_attn_decode_shared_splits with n = Q: ceil(T / (B * ceil(Q/4) * Hkv)) with T = ceil(2 *
 * attn_decode_wgs / 3), at least 64 keys of Scap per slice, at least 1.                                                       */
int mm_attn_decode_verify_splits(int B, int Q, int Hkv, int Scap);
int mm_attn_decode_verify(int dtype, const void* q, const void* k, const void* v, int B, int Q, int Scap, int Sp, int Hq, int Hkv,
                          int D, int64_t q_sb, int64_t q_sh, int64_t k_sb, int64_t k_ss, int64_t k_sh, int64_t v_sb, int64_t v_ss,
                          int64_t v_sh, const int64_t* key_mask, const int32_t* base, float scale, void* out, float* workspace,
                          int nsplit, void* stream);

/* ---- Prompt-lookup speculative decoding (generate's prompt_lookup_num_tokens = k; opt-in; greedy only).  transformers'
 * PromptLookupCandidateGenerator.get_candidates per row, for `rows` <= 16 rows at once, and the bookkeeping of a verify step, all on
 * the device.  Row state (int32, device): hist [rows, ld_hist] the visible prompt ids followed by every emitted id (mm_logits_process'
 * layout), hlen[r] its length, count[r] ids emitted so far, finished[r] (0 / 1: eos emitted), base[r] the position and cache slot of
 * the row's newest id.  A row is ACTIVE iff finished[r] == 0 and count[r] < max_new.
 *
 * mm_lookup_draft: with h = hist[r], L = hlen[r] (clamped into [0, ld_hist]; L >= 1 is the caller's contract):
 *   for g = min(max_ngram, L - 1) down to 1: the FIRST i (ascending) in [0, L - g) with h[i .. i+g) == h[L-g .. L) wins, at the largest
 *   g that has one (windows may overlap the tail; i + g < L, so at least one id follows).  start = i + g; the candidate is
 *   h[start .. min(start + k, L)), cut before its first eos (an empty result means no draft: no other match is tried, as in HF), then
 *   clipped to max_new - count[r] - 1 ids.  n_draft[r] = its length, 0 for a row that is not active.
 *   ids[r, 0] = h[L-1], ids[r, 1 .. n_draft] = the draft, the remaining columns repeat ids[r, 0]; pos[r, j] = base[r] + j.  ids, pos:
 *   int64 [rows, k+1] contiguous.  One workgroup per row; the first match is an integer min-reduction: the same result on every launch.
 *   MM_ERR_ARG before any launch: a NULL pointer, rows outside [0, 16], k outside [1, 15], max_ngram < 1, max_new < 1, ld_hist < 1.
 *
 * mm_kv_append_at: the roped k heads and the v heads of x [B*Q, ld] (a fused q|k|v row of (Hq + 2 Hkv) * D elements, MM_BF16, row
 *   b*Q + j) are copied to kcache / vcache [B, Smax, Hkv, D] (element strides c_sb per sequence, c_ss per slot, D per head) at slot
 *   base[b] + j: the bits LayerKVCache.store writes.  A slot outside [0, Smax) is skipped: nothing is written for it.
 *   MM_ERR_ARG: a NULL pointer, B < 0, Q outside [1, 16], Hq < 1, Hkv < 1, Smax < 1, ld < (Hq + 2 Hkv) * D, c_ss < Hkv * D, c_sb < Smax * c_ss (B > 1); MM_ERR_UNSUPPORTED: another
 *   dtype, D % 8 != 0; MM_ERR_ALIGN: ld, c_sb or c_ss not a multiple of 8 elements, x / kcache / vcache not 16-byte aligned.
 *
 * mm_lookup_accept: tok int64 [rows, Q] is the model's own choice behind every verify position (Q = k + 1; Q = 1 with ids and n_draft
 *   NULL: the prefill's token, a verify step without drafts).  Per ACTIVE row: a = the number of leading j < n_draft[r] (clamped into
 *   [0, Q - 1]) with ids[r, 1+j] == tok[r, j]; tok[r, 0 .. a] are emitted in order, stopping after the first eos (finished[r] = 1) or
 *   when count[r] reaches max_new.  The m >= 1 emitted ids go to out[r, count[r] ..] (int64 [rows, ld_out], ld_out >= max_new) and to
 *   hist[r, hlen[r] ..] (an index >= ld_hist is not written); count, hlen and base each grow by m; stats[r] += (1, m - 1) (int32
 *   [rows, 2]: verify steps, accepted drafts).  A row that is not active changes nothing.  done[0] = 1 iff no row is active after the
 *   call, else 0.  One workgroup.  MM_ERR_ARG before any launch: a NULL pointer (ids / n_draft: only when Q > 1), rows outside [0, 16],
 *   Q outside [1, 16], max_new < 1, ld_out < max_new, ld_hist < 1.
 * All three: no allocation, copy or synchronisation inside (capturable); rows / B = 0: MM_OK, nothing written.                    */
int mm_lookup_draft(const int32_t* hist, int ld_hist, const int32_t* hlen, const int32_t* count, const int32_t* finished,
                    const int32_t* base, int rows, int k, int max_ngram, int max_new, int64_t eos, int64_t* ids, int64_t* pos,
                    int32_t* n_draft, void* stream);
int mm_kv_append_at(int dtype, const void* x, int ld, int B, int Q, int Hq, int Hkv, int D, const int32_t* base, void* kcache,
                    void* vcache, int64_t c_sb, int64_t c_ss, int Smax, void* stream);
int mm_lookup_accept(const int64_t* tok, const int64_t* ids, const int32_t* n_draft, int rows, int Q, int max_new, int64_t eos,
                     int64_t* out, int ld_out, int32_t* hist, int ld_hist, int32_t* hlen, int32_t* count, int32_t* finished,
                     int32_t* base, int32_t* stats, int32_t* done, void* stream);

/* ---- Beam search selection on the device (generate's num_beams = n; opt-in).  transformers' GenerationMixin._beam_search with one
 * eos token, no logits processors and do_sample = False, restated without its -1e9 arithmetic.  Per prompt b the state is n running
 * beams (fp32 score s[j] and a sequence), a finished set F of at most n entries (normalised score, sequence, length) and a flag
 * open[b], initially true.  T = max_new_tokens, R = B*n.  mm_beam_step(step = i) -- i tokens generated so far -- does:
 *  a. lp[j,v] = s[j] + (x[j,v] - lse_j) in fp32, x = float(logits[row j, v]) (-0 counts as +0), lse_j = m + logf(sum_v expf(x - m))
 *     with m the row's maximum, summed per 4096-entry chunk and then over the chunks in chunk order.  Step 0 reads ONE row per prompt
 *     (logits [B, ld], the prefill's), j = 0 and s = 0; every later step reads logits [B*n, ld], row b*n + j.  Columns [V, ld) are
 *     never read.  A -inf logit (lp = -inf) is never chosen; a prompt must offer at least 2n finite lp.
 *  b. C = the 2n largest lp of the prompt, descending.  Ties go to the smaller flat index j*V + v; where fp32 rounding has collapsed
 *     two different logits of ONE row to the same lp, the larger logit goes first (exact same-row ties are equal logits, and those
 *     go to the smaller token).  A candidate carries (parent j, token v, score lp).
 *  c. stop[c] = (v == eos) or (i + 1 == T).
 *  d. The next running beams are the first n candidates with stop false, in order: next_ids[b*n + r] (int64, the next embedding
 *     lookup), parent, score.  At the last step there are none: next_ids = eos, parent r, score -inf, and s_new[0] of rule f is -inf.
 *  e. Skipped when open[b] is false, and when early_stopping = 1 and F held n entries BEFORE this step.  Otherwise every candidate of
 *     rank < n with stop true enters F with score lp / d_i, d_i = (float)pow(i + 1, length_penalty) (double pow, rounded once), length
 *     i + 1 and its tokens (the parent's sequence, then v); F keeps its best n: a new entry needs a score strictly above the worst
 *     entry's (on a tie the existing entry stays; among new ones the lower rank goes first), and the worst entry is the lowest score,
 *     then the latest arrival.
 *  f. If F holds n entries: open[b] &= s_new[0] / d_L > min(F), d_L = (float)pow(L, length_penalty) with L = T when
 *     early_stopping = 2 ("never") and length_penalty > 0, else L = i + 1.  Otherwise open[b] stays.
 *  g. done = no prompt is open, or early_stopping = 1 and every F holds n entries, or i + 1 == T.
 * After done, further steps leave every F unchanged (rule e skips them: a closed prompt stays closed, a full F stays full), so the
 * host may look at done only every few steps.  early_stopping: 0 False, 1 True, 2 "never".
 * The step also writes the ancestor table of the COMING decode step for mm_attn_decode_beam: anc_new[t][r] = anc_old[t][b*n +
 * parent[r]] for t < i and anc_new[i][r] = r (the slot that step appends to); two tables ping-pong, step i reads table i & 1 and
 * writes table (i + 1) & 1 (entries are physical rows, clamped into the prompt's rows when read).  Sequences are not copied per
 * step: token t of running beam r is tok[t][anc[t][r]].
 * state: mm_beam_state_bytes(B, n, T) bytes, 16-byte aligned, owned by the caller for the whole call of generate; step 0 starts it
 * (nothing needs clearing).  mm_beam_state_layout writes the byte offsets of its 11 fields: 0 score f32 [R], 1 parent i32 [R] (of the
 * last step, relative to the prompt's first row), 2 tok i32 [T,R], 3 anc i32 [2,T,R] (anc_ld = R), 4 fscore f32 [R], 5 flen i32 [R]
 * (0: empty slot), 6 fseqno i32 [R] (arrival number), 7 fseq i32 [R,T], 8 open i32 [B], 9 fcount i32 [B] (arrivals so far;
 * min(fcount, n) slots hold entries), 10 done i32 [1].  F's slots are not kept sorted.
 * ws: mm_beam_ws_bytes(B, n, V) bytes, 16-byte aligned, scratch of one step.  logits MM_BF16 or MM_F32, row stride ld >= V.
 * Three short launches (per-row chunk maxima / sums / top-2n; one workgroup per prompt for b-f; g), no allocation, no host sync,
 * no atomics: the same bits on every launch.
 * MM_ERR_ARG before any launch: n outside [1, 16], B < 1, B*n > 65535, V < 2n or V > 2^24, ld < V, step outside [0, T), T < 1,
 * early_stopping outside {0, 1, 2}, length_penalty not finite, a NULL pointer, a short state or ws; MM_ERR_ALIGN: state or ws not
 * 16-byte aligned.
 * mm_beam_finish: ranks every prompt's F (higher score, then the earlier arrival) and writes its num_return <= n best: ids int64
 * [B*num_return, T] (row b*num_return + k; eos behind the hypothesis' end), scores f32 and lens i32 [B*num_return].              */
int mm_beam_ws_bytes(int B, int n, int V, int64_t* bytes);
int mm_beam_state_bytes(int B, int n, int max_new_tokens, int64_t* bytes);
int mm_beam_state_layout(int B, int n, int max_new_tokens, int64_t* offsets);
int mm_beam_step(int dtype, const void* logits, int B, int n, int V, int ld, int step, int max_new_tokens, int64_t eos,
                 float length_penalty, int early_stopping, void* state, int64_t state_bytes, void* ws, int64_t ws_bytes,
                 int64_t* next_ids, void* stream);
int mm_beam_finish(const void* state, int64_t state_bytes, int B, int n, int max_new_tokens, int num_return, int64_t eos,
                   int64_t* ids, float* scores, int32_t* lens, void* stream);

/* ---- MXFP8 KV cache for the decode step (opt-in).  The K and V rows [Hkv, D] of every cached position, D = 128 only, are stored in
 * the format of mm_quant_mxfp8 above: OCP e4m3fn elements, one E8M0 scale byte per 32 consecutive d of a head (4 per (position, kv
 * head) for K and 4 for V), the same quantiser rule -- the smallest scale that keeps the block maximum <= 448, byte clamp [27, 254],
 * 127 for a zero block, round to nearest even, sign of zero kept.  1 + 1/32 byte per element, 0.516 of bf16; the rows the buffer stands
 * for are ordinary bf16 tensors, exactly.  One buffer per layer holds K and V of [B, Smax] positions; its layout is private to the
 * library (csrc/mm_kv8.h), fixed by (B, Smax, Hkv); the buffer is 16-byte aligned (MM_ERR_ALIGN).  MM_BF16 and D = 128, else
 * MM_ERR_UNSUPPORTED; non-positive sizes and NULL operands are MM_ERR_ARG.  All checks come before any launch.
 * mm_kv8_bytes:    bytes of one layer's buffer (K and V, elements and scales), a multiple of 16, with
 *                  2*B*Smax*Hkv*132 <= bytes <= 2*B*round_up(Smax,16)*Hkv*132 + 64; negative MM_ERR_UNSUPPORTED / MM_ERR_ARG.
 * mm_kv8_append:   quantises the bf16 rows k / v [b, s, h, :] (strides in elements: k_sb, k_ss, v_sb, v_ss, head stride D -- strided
 *                  views into a fused q|k|v row; multiples of 8 and k, v 16-byte aligned, else MM_ERR_ALIGN) into positions
 *                  pos .. pos + S - 1.  One pass, both tensors in one launch; S = the prompt length at prefill, 1 in a decode step.
 *                  Nothing outside those positions is written.  MM_ERR_ARG if pos < 0 or pos + S > Smax.
 * mm_kv8_dequant:  the bf16 rows of positions pos .. pos + S - 1, exactly, into k_out / v_out [B, S, Hkv, D] (both with batch stride sb
 *                  and position stride ss, multiples of 8; head stride D).  For tests and debugging.
 * mm_attn_decode_kv8_chunk: keys per slice of mm_attn_decode_kv8 = ceil(Skv / nsplit) rounded up to the layout's alignment (a power
 *                  of two <= 16, csrc/mm_kv8.h): slice s holds keys [s*chunk, min(Skv, (s+1)*chunk)).  MM_ERR_ARG for Skv <= 0 or nsplit < 1.
 * mm_attn_decode_kv8: mm_attn_decode's two-launch form (sync = NULL) over the buffer: q, key_mask, out, workspace and nsplit as there
 *                  (nsplit from mm_attn_decode_splits; any nsplit >= 1 is accepted), Skv <= Smax cached positions.  D = 128 and Hq/Hkv
 *                  in {1, 2, 4} (MM_ERR_UNSUPPORTED otherwise).  Whenever the slices coincide -- nsplit == 1, or ceil(Skv / nsplit) a
 *                  multiple of the alignment -- out is bit-identical to mm_attn_decode run on mm_kv8_dequant's rows with the same nsplit
 *                  (the slice kernel is the same code: the stored bytes become the same MFMA operands).  Every slice's record is
 *                  written, an empty slice's included.  The result does not depend on anything stored for positions >= Skv: slots
 *                  never appended to may hold any bytes.                                                                           */
int64_t mm_kv8_bytes(int B, int Smax, int Hkv, int D);
int mm_kv8_append(int dtype, const void* k, const void* v, int B, int S, int Hkv, int D, int64_t k_sb, int64_t k_ss, int64_t v_sb,
                  int64_t v_ss, void* cache, int Smax, int pos, void* stream);
int mm_kv8_dequant(const void* cache, int B, int Smax, int Hkv, int D, int pos, int S, void* k_out, void* v_out, int64_t sb, int64_t ss,
                   void* stream);
int mm_attn_decode_kv8_chunk(int Skv, int nsplit);
int mm_attn_decode_kv8(int dtype, const void* q, const void* cache, int B, int Skv, int Smax, int Hq, int Hkv, int D, int64_t q_sb,
                       int64_t q_sh, const int64_t* key_mask, float scale, void* out, float* workspace, int nsplit, void* stream);

/* ---- activations -----------------------------------------------------------------------------------------
 * SwiGLU: HF:llama:163-176.  gu [M, 2I] = [gate | up] from the fused gate/up GEMM; out [M,I] = silu(gate)*up.
 * Rounding points of the forward (T = the storage type): out = T(f32(T(silu(gate))) * up): silu(gate) is rounded to T BEFORE the
 * multiply by up, as HF's act_fn(gate_proj(x)) * up_proj(x) in the storage dtype.  The backward rounds each output once.        */
int mm_swiglu_fwd(int dtype, const void* gu, int M, int I, void* out, void* stream);
int mm_swiglu_bwd(int dtype, const void* gu, const void* dout, int M, int I, void* dgu, void* stream);
/* xIELU (Apertus MLP: down_proj(xIELU(up_proj(h))); HF 5.15 activations.py XIELUActivation._xielu_python).  x = the pre-activation,
 * n elements, T = the storage type, all arithmetic fp32:
 *   sp(a) = a > 20 ? a : log1p(exp(a));   ap = sp(*alpha_p_raw),  an = beta + sp(*alpha_n_raw)
 *   y  = x > 0 ? ap x^2 + beta x : an (expm1(min(x, eps)) - x) + beta x
 *   dx = dy * (x > 0 ? 2 ap x + beta : an (m(x) exp(x) - 1) + beta),  m = 1 below eps, 1/2 at eps, 0 above (torch.min's tie rule)
 *   dalpha_p_raw = sp'(*alpha_p_raw) * sum_{x > 0} dy x^2,   dalpha_n_raw = sp'(*alpha_n_raw) * sum_{x <= 0} dy (expm1(min(x, eps)) - x)
 * alpha_*_raw: one element of T each in device memory (no host sync).  beta / eps: the values of the model's buffers (in a bf16
 * model the bf16-rounded ones).  y and dx are rounded once to T.  x, y, dy, dx 16-byte aligned (MM_ERR_ALIGN); any n >= 0.
 * mm_xielu_bwd: partials = f32 [mm_xielu_bwd_blocks(n), 2] (8-byte aligned), the workgroups' sums of the two scalar gradients' terms;
 *   NULL = the scalars are frozen: dx only.  mm_xielu_bwd_blocks depends on n alone (never on the device).
 * mm_xielu_reduce: adds the nblk partials in a fixed order in fp32, applies sp', and writes -- or, where accumulate_* is set, adds
 *   in fp32 to the existing T value -- the two gradients, rounded once.  No atomics anywhere: equal inputs give equal bits.          */
int mm_xielu_fwd(int dtype, const void* x, int64_t n, const void* alpha_p_raw, const void* alpha_n_raw, float beta, float eps, void* y,
                 void* stream);
int mm_xielu_bwd_blocks(int64_t n);
int mm_xielu_bwd(int dtype, const void* x, const void* dy, int64_t n, const void* alpha_p_raw, const void* alpha_n_raw, float beta,
                 float eps, void* dx, float* partials, void* stream);
int mm_xielu_reduce(int dtype, const float* partials, int nblk, const void* alpha_p_raw, const void* alpha_n_raw, void* dalpha_p_raw,
                    void* dalpha_n_raw, int accumulate_p, int accumulate_n, void* stream);
/* kind: 0 = erf GELU (mlp.py:35,37), 1 = quick GELU (HF:clip fc1).  x is the pre-activation.                       */
/* kind: 0 = erf GELU, 1 = quick GELU, 2 = tanh GELU */
int mm_gelu_fwd(int dtype, int kind, const void* x, int64_t n, void* y, void* stream);
int mm_gelu_bwd(int dtype, int kind, const void* x, const void* dy, int64_t n, void* dx, void* stream);
/* y = a + b (residual adds that are not fused into a GEMM epilogue)                                             */
int mm_add(int dtype, const void* a, const void* b, int64_t n, void* y, void* stream);

/* ---- loss: HF:loss/loss_utils.py:36-71 --------------------------------------------------------------------------
 * logits [T, ld] (V valid columns; [V, ld) is never read); labels already shifted by the caller; ignore_index = -100.
 * Which rows are live, one rule for the three kernels: a NEGATIVE label (-100, and any other negative value) is ignored: its
 * loss_row is 0, its dlogits row is 0 and it is not counted.  A label in [0, V) is live and counted.  A label >= V is a caller
 * error that is not diagnosed: the row gives no loss and no gradient (mm_ce_fwd / mm_ce_bwd see V) but mm_ce_reduce, which
 * does not know V, counts it.  The callers in functional.py produce -100 or token ids below V only.
 * -inf logits (masked vocabulary entries) count as exp = 0 wherever they stand in the row; a row needs at least one finite logit
 * and a finite logit at its label (otherwise lse / loss_row are -inf / NaN: out of contract).
 * fwd: lse[T] f32, loss_row[T] f32 (0 for ignored rows).  loss = sum(loss_row)/count is reduced by mm_ce_reduce.    */
int mm_ce_fwd(int dtype, const void* logits, int T, int V, int ld, const int64_t* labels, float* lse, float* loss_row, void* stream);
/* out[0] = sum(loss_row)/max(count,1), out[1] = count (number of labels >= 0; see the rule above)                    */
int mm_ce_reduce(const float* loss_row, const int64_t* labels, int T, float* out, void* stream);
/* dlogits[t,v] = (exp(logit - lse[t]) - [v==label]) * gscale[0] / count, 0 for ignored rows and for v in [V, ld)    */
int mm_ce_bwd(int dtype, const void* logits, int T, int V, int ld, const int64_t* labels, const float* lse,
              const float* loss_and_count, const float* gscale, void* dlogits, void* stream);
/* next-token selection of model.py:607-621: argmax(softmax(logits/T)) over the LAST dim, first max wins.
 * Rounding points (T = the storage type), chosen so that ties resolve as torch.argmax over the softmax tensor in the logits
 * dtype does: s = T(x / temperature) (fp32 division), p = T(exp(s - max s) / sum exp(s - max s)) with fp32 softmax arithmetic,
 * result = the FIRST index of the maximum of p.  temperature > 0 (MM_ERR_ARG otherwise); any row stride ld >= V.              */
int mm_argmax_softmax(int dtype, const void* logits, int rows, int V, int ld, float temperature, int64_t* out, void* stream);
/* the same selection for long rows, the vocabulary cut into chunks over many workgroups (3 short launches instead of one block per
 * row sweeping 128 258 logits three times); ws: mm_argmax_softmax_ws_bytes(rows, V) bytes, 8-byte aligned                     */
int mm_argmax_softmax_ws_bytes(int rows, int V);
int mm_argmax_softmax_split(int dtype, const void* logits, int rows, int V, int ld, float temperature, int64_t* out, void* ws,
                            void* stream);
/* Seeded next-token sampling (generate(do_sample=True, top_k=, top_p=, min_p=, seed=); HF warper order temperature -> top-k ->
 * top-p -> min-p, HF:generation/utils.py).  Per row r of logits [rows, ld] (V valid columns), in fp32:
 *   1. x_v = float(logit_v) / T;  m = max_v x_v;  w_v = exp(x_v - m)
 *   2. top-k (0 or >= V: off): keep x_v >= x_(k), the k-th largest value; ties at it are all kept (TopKLogitsWarper)
 *   3. top-p (1: off), over the set kept so far with mass Z_K: keep v iff sum of w_u over kept u with x_u > x_v < top_p * Z_K
 *      (TopPLogitsWarper, min_tokens_to_keep = 1, ties resolved by value: kept together); the maximum is always kept
 *   4. min-p (0: off): keep v iff w_v >= min_p  (p_v >= min_p * p_max, MinPLogitsWarper)
 *   5. u = (philox4x32_10(call = r, offset, seed).x >> 8) * 2^-24 in [0, 1), t = u * Z with Z the kept mass: the token is the
 *      smallest kept index v (vocabulary order) whose cumulative kept mass C(v) > t; if rounding leaves none, the last kept one
 *   6. x = -inf is never drawn; a row without a finite logit is out of contract but still gets an index in [0, V)
 *   7. bitwise deterministic: the mass is fixed point (w * 2^38 as an integer; sums exact in any order), no float atomics
 * thresh (may be NULL): the smallest kept x of each row.  ws: mm_sample_ws_bytes(rows, V) bytes, 16-byte aligned; V <= 2^24.
 * MM_ERR_ARG before any launch for T <= 0, top_k < 0, top_p outside (0, 1] or NaN, min_p outside [0, 1], ld < V, rows < 0 or
 * a workspace that is too small.  No allocation, copy or synchronisation inside (capturable).
 * mm_sample_uniforms: the u of step 5 for rows 0 .. rows-1 (tests).                                                       */
int mm_sample_ws_bytes(int rows, int V, int64_t* bytes);
int mm_sample(int dtype, const void* logits, int rows, int V, int ld, float temperature, int top_k, float top_p, float min_p,
              int64_t seed, int64_t offset, int64_t* out, float* thresh, void* ws, int64_t ws_bytes, void* stream);
int mm_sample_uniforms(int64_t seed, int64_t offset, int rows, float* u, void* stream);
/* generate()'s per-token bookkeeping ON the device (the reference syncs per token: model.py:618-625,637-638): id = finished[b]
 * ? eos : tok[b]; finished[b] |= id == eos; out[b, col] = id; next_ids[b] = id (the next step's embedding lookup).  Nothing
 * else is written (out [B, ld_out]: column col only).  MM_ERR_ARG: a NULL pointer, B < 0, col outside [0, ld_out); B = 0: MM_OK. */
int mm_decode_select(const int64_t* tok, unsigned char* finished, int64_t eos, int B, int64_t* out, int ld_out, int col,
                     int64_t* next_ids, void* stream);
/* generate()'s logits processors (repetition_penalty=, no_repeat_ngram_size=, min_new_tokens=, suppress_tokens=) in one launch per
 * step, between lm_head and the selection: logits [rows, ld] (MM_BF16 / MM_F32, V valid columns) -> out fp32 [rows, ld_out].
 * Row history: hist int32 [rows, ld_hist]; the caller filled row r's plen[r] prompt ids (0 <= plen[r] <= max_plen; clamped) at
 * hist[r, 0 .. plen[r]).  At step = i row r's history h has L = plen[r] + i entries; a call with i > 0 first stores
 * (int32)last_ids[r] -- the id the previous step emitted, mm_decode_select's next_ids -- at hist[r, plen[r] + i - 1], so that it and
 * every later call see it.  Calls are made with step = 0, 1, 2, ... (not checked); nothing else of hist is written.  History
 * entries outside [0, V) never index a row: they are not penalised and not banned (as plain integers they still take part in the
 * n-gram comparison of rule 2).
 * Per row, x_v = float(logits[r, v]), fp32 arithmetic, p = repetition_penalty, in transformers' order (RepetitionPenalty ->
 * NoRepeatNGram -> MinNewTokensLength -> SuppressTokens LogitsProcessor on fp32 scores):
 *   1. p != 1: for every v that occurs in h, ONCE however often it occurs: x_v = x_v < 0 ? x_v * p : x_v / p (correctly rounded
 *      division; -0 is not < 0, so -0 / p = -0; -inf stays -inf)
 *   2. g = no_repeat_ngram_size > 0 and L + 1 >= g: for every i in [0, L - g] with h[i .. i+g-2] == h[L-g+1 .. L-1]:
 *      x_{h[i+g-1]} = -inf  (g = 1: the empty tail, every id of h is banned)
 *   3. step < min_new_tokens: x_eos = -inf
 *   4. x_t = -inf for every t of suppress[0 .. n_suppress) (int32, device memory) inside [0, V); duplicates allowed
 *   5. out[r, v] = x_v for v < V.  Columns [V, ld_out) of out are never written, columns [V, ld) of logits never read; out must
 *      not overlap logits.
 * hist and plen may be NULL iff p == 1 and g == 0 (no history is kept then and last_ids is not read); with hist given the newest id
 * is stored whatever p and g are.  A row left without a finite score is out of contract, as for mm_sample.  Bitwise deterministic
 * (integer LDS atomics only); no allocation, copy or synchronisation inside (capturable).
 * MM_ERR_ARG before any launch: p not finite or <= 0, g < 0, min_new_tokens < 0, step < 0, eos outside [0, V) while step <
 * min_new_tokens, V <= 0, ld < V, ld_out < V, rows < 0, n_suppress < 0, max_plen < 0 or max_plen + step > ld_hist (hist given), a
 * required pointer that is NULL (logits, out; suppress when n_suppress > 0; hist and plen when p != 1 or g > 0; plen, and last_ids
 * when step > 0, when hist is given), out == logits.  rows = 0: MM_OK.                                                          */
int mm_logits_process(int dtype, const void* logits, int rows, int V, int ld, int step, const int64_t* last_ids, int32_t* hist,
                      int ld_hist, const int32_t* plen, int max_plen, float repetition_penalty, int no_repeat_ngram_size,
                      int min_new_tokens, int64_t eos, const int32_t* suppress, int n_suppress, float* out, int ld_out,
                      void* stream);
/* generate()'s classifier-free guidance (guidance_scale=; opt-in): transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor, the
 * first processor of HF's chain, from the conditional and the unconditional logits of one step to the fp32 scores every later
 * processor and selector reads.  cond [rows, ld_c] and uncond [rows, ld_u] (MM_BF16 / MM_F32, V valid columns; columns [V, ld) are
 * never read): row r of uncond is the unconditional row of row r of cond.  out fp32 [rows, ld_out]; columns [V, ld_out) are never
 * written; out overlaps neither input.
 * Per row and per operand, in fp32: x_v = float(logit_v); lse = m + logf(sum_v expf(x_v - m)) by mm_beam_step's rule a -- per
 * 4096-entry chunk with the chunk's own maximum, then over the chunks in chunk order with m the row's maximum --; y_v = x_v - lse.
 *   out_v = fl(fl(scale * fl(yc_v - yu_v)) + yu_v)
 * the three operations rounded separately, never a fused multiply-add: HF's scores = uncond + scale * (cond - uncond) on the two
 * log_softmax rows, operation for operation (bit-equal rows of a pair give yc - yu = 0 exactly, hence out = yu at every scale).
 * Domain: scale finite, logits finite.  A -inf or NaN logit is out of contract; it still touches nothing outside out[:, :V].
 * Two launches (chunk maxima and sums over 2 rows x ceil(V / 4096) workgroups, then the combine over rows x ceil(V / 4096));
 * bitwise deterministic: no atomics, no arrival counters, fixed reduction orders.  No allocation, copy or synchronisation inside
 * (capturable).  16-byte vector loads / stores where the base and the row stride allow, scalar ones otherwise.
 * ws: mm_cfg_ws_bytes(rows, V) bytes (the partials), 16-byte aligned.
 * MM_ERR_ARG before any launch: another dtype, rows < 0 or > 32767, V <= 0 or V > 2^24, ld_c < V, ld_u < V, ld_out < V, a scale
 * that is not finite, a NULL pointer (cond, uncond, out, ws; bytes of mm_cfg_ws_bytes), ws_bytes too small, out == cond or out ==
 * uncond.  MM_ERR_ALIGN: ws not 16-byte aligned.  rows = 0: MM_OK, nothing written.                                           */
int mm_cfg_ws_bytes(int rows, int V, int64_t* bytes);
int mm_cfg_combine(int dtype, const void* cond, int ld_c, const void* uncond, int ld_u, int rows, int V, float scale,
                   float* out, int ld_out, void* ws, int64_t ws_bytes, void* stream);

/* ---- MoE image modality: gating-weighted fusion of the experts' token features (modalities/image_modality_moe.py:163-205)
 * X [E, n, L] (L = P*C, expert-major), gate [n, E] fp32 (the gating network's softmax weights, expert order), idx[J] = the
 * experts taking part (host array).  mode 0: out[n, L] = sum_j gate[n, idx[j]] * X[idx[j], n]  (`weighted_average`, :170-176);
 * mode 1: out[n, J, L] = softmax_j(gate[n, idx[.]])[j] * X[idx[j], n]  (the specialists' scaled contexts of `cross_attn`,
 * :186-199).  backward = 1: X is d(out), out is dX [E, n, L]: dX[idx[j], n] = w_j * dout[n] (mode 0) / w'_j * dout[n, j] (mode 1);
 * only the listed experts' slices are written, the unlisted slices are not touched (the caller zeroes them).
 * Rounding: the weights, the J-way softmax and the sum are fp32 arithmetic; each output element is rounded ONCE to the dtype.
 * MM_ERR_ARG: J outside 1 .. 16, an index outside [0, E), mode outside {0, 1}, a NULL pointer; MM_ERR_ALIGN: L not a multiple of
 * the 16-byte vector (8 bf16 / 4 f32), X or out not 16-byte aligned; n = 0: MM_OK, nothing written.                        */
int mm_expert_fuse(int dtype, int backward, int mode, const void* X, const float* gate, const int* idx, int J, int E, int n,
                   int64_t L, void* out, void* stream);

/* ---- MoE image modality: the core of `CrossAttention` (model/attention.py:79-96: softmax(q k^T * scale) -> attn_drop -> @ v,
 * called with the generalist's P tokens as queries over the specialists' (E-1)*P tokens, image_modality_moe.py:177-203 and
 * image_modality_moe_pep.py:216-244) for head widths the flash kernels do not tile: any D that is a multiple of 8 up to 512
 * (MM_BF16; the shipped recipes need 96 = 768/8 and 512 = 4096/8), any D for MM_F32; Nkv <= 1024 (the whole score row of a
 * query stays in registers: no online softmax).  q [n,Nq,H,D], k/v [n,Nkv,H,D] with element strides (image, token, head);
 * out [n,Nq,H,D] contiguous; lse [n,H,Nq] f32.  drop_p = probability of zeroing an attention weight (`attn_drop`, 0.1 in the
 * reference whenever the module trains; 0 = eval): Philox4x32-10 with key `seed` and counter (call, offset); weight (row, key)
 * with row = (image * H + head) * Nq + query takes component key & 3 of call row * KP/4 + key/4, KP = Nkv rounded up to 32
 * (mm_dropout_mask(seed, offset, rows * KP, p) lists the same keep flags).  Backward regenerates the mask, is deterministic
 * (no atomics) and needs a workspace of mm_xattn_ws_bytes; dq/dk/dv take the strides of q/k/v.                            */
int mm_xattn_ws_bytes(int dtype, int n, int Nq, int Nkv, int H, int64_t* bytes);
int mm_xattn_fwd(int dtype, const void* q, const void* k, const void* v, int n, int Nq, int Nkv, int H, int D, int64_t q_sb,
                 int64_t q_ss, int64_t q_sh, int64_t k_sb, int64_t k_ss, int64_t k_sh, int64_t v_sb, int64_t v_ss, int64_t v_sh,
                 float scale, float drop_p, int64_t seed, int64_t offset, void* out, float* lse, void* stream);
int mm_xattn_bwd(int dtype, const void* q, const void* k, const void* v, const void* out, const void* dout, const float* lse,
                 int n, int Nq, int Nkv, int H, int D, int64_t q_sb, int64_t q_ss, int64_t q_sh, int64_t k_sb, int64_t k_ss,
                 int64_t k_sh, int64_t v_sb, int64_t v_ss, int64_t v_sh, float scale, float drop_p, int64_t seed, int64_t offset,
                 void* dq, void* dk, void* dv, void* ws, int64_t ws_bytes, void* stream);
/* y[i] = keep(i) ? x[i] / (1 - p) : 0 -- nn.Dropout of CrossAttention's output projection (attention.py:41,98, `proj_drop`);
 * element i takes component i & 3 of Philox call i / 4.  Its backward is the same call on dy with the same (seed, offset).
 * mm_dropout_mask: the keep flags (uint8 0/1) of elements 0 .. n-1 of that stream (tests).                                */
int mm_dropout(int dtype, const void* x, int64_t n, float p, int64_t seed, int64_t offset, void* y, void* stream);
int mm_dropout_mask(int64_t seed, int64_t offset, int64_t n, float p, void* mask_u8, void* stream);

/* ---- MoE image modality: the gating network, a ResNet-50 in eval mode (moe/gating.py:37-89 = torchvision resnet50 with an E-way
 * fc; model/modalities/gating.py).  Activations are NHWC: the channel dimension is contiguous, so every filter tap of every
 * pixel is a run of 16-byte vectors.  Storage type T = bf16 (MM_BF16, fp32 accumulation) or fp32 (MM_F32, the parity path).
 * mm_nchw_to_nhwc: pixels f32 [n, C, H, W] -> out T [n, H, W, Cpad], channels C .. Cpad-1 written as zeros (the stem's 3 -> 8
 *   padding; its weight is zero-padded to match).  Cpad >= C and Cpad % 8 == 0 (bf16) / % 4 (f32), out 16-byte aligned
 *   (MM_ERR_ALIGN otherwise).
 * mm_conv2d_nhwc_fwd: y[n, Ho, Wo, Cout] = act(conv(x[n, H, W, Cin], w[Cout, R, R, Cin]) * scale[Cout] + shift[Cout]
 *   (+ residual[n, Ho, Wo, Cout])), Ho = (H + 2 pad - R) / stride + 1 (Wo alike), zero padding, act = ReLU (relu != 0) or nothing;
 *   w is the filter packed [Cout, R, S, Cin] (K = R*S*Cin contiguous), scale / shift are fp32 (eval-mode BatchNorm as a per-channel
 *   affine: it is NOT folded into the weights), residual may be NULL.  An implicit GEMM with M = n*Ho*Wo, N = Cout, K = R*R*Cin
 *   (MM_BF16: v_mfma_f32_32x32x16_bf16); out-of-image taps count as zeros and nothing outside x is read.  Rounding points: exact
 *   bf16 products accumulated in fp32 (any order), then acc * scale + shift (one fma) (+ residual) (ReLU) in fp32 and ONE rounding
 *   to T at the store (mm_gemm's epilogue rule).  R in {1, 3, 7}, stride in {1, 2}, pad in {0, 1, 3} (MM_ERR_UNSUPPORTED otherwise);
 *   Cin % 8 == 0, Cout % 64 == 0 and x, w, scale, shift, residual, y 16-byte aligned (MM_ERR_ALIGN otherwise); M <= 2^31 - 257 and
 *   Cout * K < 2^31 (MM_ERR_UNSUPPORTED above); a filter larger than the padded image is MM_ERR_ARG.  M is arbitrary (ragged last
 *   tiles).  All checks come before any launch.
 * mm_maxpool2d_nhwc: y[n, Ho, Wo, C] = max over the 3x3 window, stride 2, pad 1 (Ho = (H - 1) / 2 + 1): ResNet's pool.  Padding
 *   taps do not take part in the maximum.  C % 8 == 0 (bf16) / % 4 (f32), x and y 16-byte aligned (MM_ERR_ALIGN otherwise).
 * mm_gate_head: the tail of the network in one launch (avgpool + fc + softmax + topk, gating.py:85-87).  x T [n, HW, C];
 *   pooled = fp32 mean over HW (sum in order, times 1/HW; NOT rounded to T); logits[n, E] = T(pooled . fc_w[E, C]^T + fc_b) with
 *   an fp32 dot product; weights[n, E] = T(softmax_fp32(float(logits))): the softmax of the ROUNDED logits, as softmax(logits) in
 *   the model dtype; topk_idx int64 [n, top_k] = indices of the top_k largest (rounded) logits, descending, the lower index first
 *   on ties.  fc_w, fc_b, logits, weights are T.  1 <= top_k <= E (MM_ERR_ARG otherwise); E <= 64 and C <= 8192
 *   (MM_ERR_UNSUPPORTED above); C % 8 == 0 (bf16) / % 4 (f32), x and fc_w 16-byte aligned (MM_ERR_ALIGN otherwise).           */
int mm_nchw_to_nhwc(int dtype, const float* pixels, int n, int C, int H, int W, int Cpad, void* out, void* stream);
int mm_conv2d_nhwc_fwd(int dtype, const void* x, int n, int H, int W, int Cin, const void* w, int Cout, int R, int stride, int pad,
                       const float* scale, const float* shift, const void* residual, int relu, void* y, void* stream);
int mm_maxpool2d_nhwc(int dtype, const void* x, int n, int H, int W, int C, void* y, void* stream);
int mm_gate_head(int dtype, const void* x, int n, int HW, int C, const void* fc_w, const void* fc_b, int E, int top_k, void* logits,
                 void* weights, int64_t* topk_idx, void* stream);

/* ---- MoE image modality: pieces of TRAINING the gating network (reference image_modality_moe.py:233-241 unfreezes it in FULL
 * mode): BatchNorm with batch statistics, forward and backward, the max-pool's backward, the convolutions' data and weight gradients
 * and the gradient of the fusion with respect to the gate weights.  T as above; every
 * entry point checks all its arguments before any launch, uses no atomics and gives the same bits on every launch.
 * mm_bn_train_fwd: z T [M, C] is the raw convolution output (mm_conv2d_nhwc_fwd with scale 1, shift 0, no residual, no ReLU: one
 *   rounding to T), M = n*Ho*Wo.  From the STORED z, in fp32: mean[C], the biased var[C] (never formed as E[z^2] - mean^2: each
 *   workgroup owns 512 rows of a 64- (bf16) / 32- (f32) channel slab and writes its own mean and its sum of squared deviations from
 *   THAT mean; the slabs are then merged in row order with the pairwise update of Chan, Golub & LeVeque 1979), invstd =
 *   1 / sqrt(var + eps); y = T(act(fma((z - mean) * invstd, gamma, beta) (+ residual))), fp32 inside, ONE rounding; act = ReLU
 *   (relu != 0) or nothing.  Summation depth: no column sum passes through more than 21 + ceil(M / 512) additions (16 in a thread,
 *   5 levels of a tree over the workgroup's 32 row groups, then the workgroups in order); tests/conv_train_check.py builds its error
 *   scale on that figure.  mean / invstd (fp32) are written for the backward.  gamma, beta, residual, y are T.  Running statistics
 *   (all three pointers may be NULL together: then none is touched) follow torch.nn.BatchNorm2d: running = (1 - momentum) * running +
 *   momentum * batch in fp32 from the stored T value, stored back in T, with the UNBIASED variance M2 / (M - 1);
 *   num_batches_tracked[0] += 1 (int64).  M < 2 is MM_ERR_ARG.  C % 64 == 0 and z, y, residual, gamma, beta, running_*, ws 16-byte
 *   aligned (MM_ERR_ALIGN otherwise); ws of mm_bn_train_ws_bytes(M, C) bytes (MM_ERR_ARG when smaller).
 * mm_bn_train_bwd: with g = dy * [y > 0] (relu != 0; y is the forward's stored output) or g = dy, and xhat = (z - mean) * invstd
 *   in fp32: dbeta = T(sum g), dgamma = T(sum g * xhat) (fp32 column sums of the depth above), dz = T(gamma * invstd * (g -
 *   sum g / M - xhat * sum(g xhat) / M)), and, where dres is not NULL (the unit had a residual input), dres = T(g): the bits of dy
 *   or zero.  Two column reductions in one pass, a merge, one elementwise pass.  Same alignment rules and workspace size.
 * mm_maxpool2d_nhwc_bwd: the backward of mm_maxpool2d_nhwc in gather form.  dx[n, h, w, c] = T(fp32 sum, in (ho, wo) row-major
 *   order, of dy[n, ho, wo, c] over the at most four windows whose maximum (n, h, w, c) is).  The maximum of a window is its FIRST
 *   maximal element in row-major window order (torch's CPU rule; post-ReLU zeros tie all the time); padding taps never win; an
 *   element that wins no window gets exactly +0.  x is the forward's input.  Alignment as the forward.
 * mm_expert_fuse_gate_bwd: d(loss) / d(gate) of mm_expert_fuse.  dgate fp32 [n, E]; experts not listed in idx get exactly 0.
 *   d[j] = sum over L of float(dout[.]) * float(X[idx[j], n, .]) (exact products, fp32 accumulation in a fixed order; dout is
 *   [n, L] in mode 0 and [n, J, L] in mode 1).  mode 0: dgate[n, idx[j]] += d[j] in the order of j.  mode 1: with w' = the softmax
 *   over the J listed weights as the forward computes it, dgate[n, idx[j]] += w'[j] * (d[j] - sum_k w'[k] d[k]).  One pass over X
 *   and dout: L is split over workgroups (fp32 partials in ws, merged in order).  ws of mm_expert_fuse_gate_bwd_ws_bytes bytes;
 *   argument rules as mm_expert_fuse, dgate and ws 16-byte aligned.
 * mm_conv2d_nhwc_dgrad: dx[n, h, w, cin] = T(sum over taps (r, s) and couts of dz[n, ho, wo, cout] * w[cout, r, s, cin] (+ addend[n,
 *   h, w, cin])), the taps being those with ho * stride - pad + r == h and wo * stride - pad + s == w inside the output image.
 *   H, W are the INPUT extents (Ho, Wo follow as in the forward); wp is the filter packed [Cin, R, S, Cout].  Exact products,
 *   fp32 accumulation (any order), the optional addend (the join of a residual branch with its identity path) added in fp32, ONE
 *   rounding.  An input pixel that no output reads gets exactly +0 (or the addend).  MM_BF16: the gather form of the forward's
 *   implicit GEMM on v_mfma_f32_32x32x16_bf16; a tap whose output coordinate is fractional or outside the image is a zero fragment
 *   and is never loaded.  R in {1, 3} (7 is MM_ERR_UNSUPPORTED: the stem needs no data gradient), stride in {1, 2}; Cin % 64 == 0,
 *   Cout % 8 == 0, all pointers 16-byte aligned (MM_ERR_ALIGN).
 * mm_conv2d_nhwc_wgrad: dw[cout, r, s, cin] (packed [Cout, R, S, Cin] as the forward's filter) = T(sum over output pixels m of
 *   dz[m, cout] * x[m @ (r, s), cin]), out-of-image taps as zeros.  The pixels are split into runs of 1024 (one workgroup row each,
 *   fp32 partials [splits, Cout, K] in ws), the runs are then added in a fixed order (mm_reduce_partials) and rounded ONCE.  MM_BF16:
 *   both MFMA operands are read transposed from row-staged LDS tiles (ds_read_b64_tr_b16).  R in {1, 3, 7}, stride in {1, 2};
 *   Cin % 8 == 0 (zero input channels, the stem's 3 -> 8 padding, give exactly 0), Cout % 64 == 0; ws of
 *   mm_conv2d_nhwc_wgrad_ws_bytes bytes = 4 * Cout * K * ceil(n Ho Wo / 1024) (MM_ERR_ARG when smaller).                          */
int mm_conv2d_nhwc_dgrad(int dtype, const void* dz, int n, int H, int W, int Cin, const void* wp, int Cout, int R, int stride, int pad,
                         const void* addend, void* dx, void* stream);
int mm_conv2d_nhwc_wgrad_ws_bytes(int n, int H, int W, int Cin, int Cout, int R, int stride, int pad, int64_t* bytes);
int mm_conv2d_nhwc_wgrad(int dtype, const void* dz, const void* x, int n, int H, int W, int Cin, int Cout, int R, int stride, int pad,
                         void* dw, void* ws, int64_t ws_bytes, void* stream);
int mm_bn_train_ws_bytes(int M, int C, int64_t* bytes);
int mm_bn_train_fwd(int dtype, const void* z, int M, int C, const void* gamma, const void* beta, const void* residual, int relu,
                    float eps, float momentum, void* y, float* mean, float* invstd, void* running_mean, void* running_var,
                    int64_t* num_batches_tracked, void* ws, int64_t ws_bytes, void* stream);
int mm_bn_train_bwd(int dtype, const void* dy, const void* y, const void* z, int M, int C, const float* mean, const float* invstd,
                    const void* gamma, int relu, void* dz, void* dres, void* dgamma, void* dbeta, void* ws, int64_t ws_bytes,
                    void* stream);
int mm_maxpool2d_nhwc_bwd(int dtype, const void* x, const void* dy, int n, int H, int W, int C, void* dx, void* stream);
int mm_expert_fuse_gate_bwd_ws_bytes(int dtype, int J, int n, int64_t L, int64_t* bytes);
int mm_expert_fuse_gate_bwd(int dtype, int mode, const void* X, const void* dout, const float* gate, const int* idx, int J, int E,
                            int n, int64_t L, float* dgate, void* ws, int64_t ws_bytes, void* stream);

/* ---- optimizer: AdamW (config_alignment.yaml:38-59 -> torch.optim.AdamW semantics) + grad-norm clip ----------------
 * sumsq partial: out[blk] = sum g^2 over a slice; mm_gradnorm_finish: total[0] = sqrt(sum) ; clip coef in total[1]
 * Contract (tests/test_optim_contract_gpu.py):
 *   mm_gradnorm_partial writes every partial[0, nblk): 16-byte vector j of g goes to block (j / 256) % nblk, the scalar tail
 *     [vn (n / vn), n) to block 0, a block without work writes exactly 0 (so does every block for n == 0).  g 16-byte aligned
 *     (MM_ERR_ALIGN); nblk <= 0, n < 0 or a NULL pointer is MM_ERR_ARG.  The same bits on every launch.
 *   mm_gradnorm_finish: total[1] = min(1, max_norm / (total[0] + 1e-6f)) for max_norm > 0, else exactly 1.  All-zero gradients
 *     give total = {0, 1}.                                                                                              */
int mm_gradnorm_partial(int dtype, const void* g, int64_t n, float* partial, int nblk, void* stream);
int mm_gradnorm_finish(const float* partial, int nblk, float max_norm, float* total, void* stream);
/* p (param dtype), g (param dtype), master/m/v f32.  clip = mm_gradnorm_finish's total (clip[1] is read, clip[0] is not) or
 * NULL for a coefficient of 1.  One step of torch.optim.AdamW on g * clip[1]: decoupled decay w (1 - lr wd), eps outside the
 * root, bias corrections bc = 1.0f - powf(beta, (float) step) evaluated in fp32 on the host -- with beta2 = 0.999 that value is
 * off from the exact one by about 1e-5 relative at steps 2 and 3 (an error of half an ulp of beta^step, amplified by
 * beta^step / bc = 499), 3e-7 at step 10, nothing at step 1 and from about step 1000; half of it reaches the update.
 * Contract: master, m, v are updated in place for all n elements (4 per thread, the tail [4 (n / 4), n) by block 0); p is
 * written, never read: p = RNE_bf16(master) (MM_BF16) or the master's bits (MM_F32).  g = m = v = 0 leaves m, v at 0 and gives
 * master (1 - lr wd).  All five pointers 16-byte aligned (MM_ERR_ALIGN); step < 1, n < 0 or a NULL pointer is MM_ERR_ARG; n == 0
 * returns MM_OK and touches nothing.  MM_ADAMW_NT=0 (read once per process) selects plain instead of non-temporal accesses
 * for bf16; mm_set_option "adamw_blocks" caps the grid (0 = default), the kernel then strides.                             */
int mm_adamw_step(int dtype, void* p, const void* g, float* master, float* m, float* v, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, const float* clip, void* stream);

/* ---- gradient exchange over RCCL (one communicator per process = per GPU) -------------------------------------------
 * Replaces the reference's DeepSpeed gradient reduce / parameter gather (config/deepspeed.json:5-19) and the NCCL process
 * group torch.distributed builds for it (cli/train.py:200-201).  RCCL is bound at run time (dlopen); without it every call
 * returns MM_ERR_UNSUPPORTED.  mm_comm_unique_id: rank 0 makes the 128-byte id, the caller carries it to the other ranks
 * (any side channel: the torchrun store, a file, MPI) and every rank calls mm_comm_init on ITS device (hipSetDevice first).
 * All collectives are in place, sum, enqueued on `stream` (asynchronous; the caller orders them with events).
 * mm_comm_allreduce_bucket algo: 0 = ncclAllReduce, 1 = reduce-scatter + all-gather in one group (shard r = rank r's; the
 * tail count % world through a small all-reduce).  mm_comm_reduce_scatter / mm_comm_all_gather: the halves on their own for
 * a sharded optimiser step (count % world == 0; shard = count / world elements at buf + rank * shard).                     */
int mm_comm_unique_id(void* id128);
int mm_comm_init(const void* id128, int rank, int world, void** comm_out);
int mm_comm_rank(void* comm, int* rank, int* world);
int mm_comm_allreduce_bucket(void* comm, int dtype, void* buf, int64_t count, int algo, void* stream);
int mm_comm_reduce_scatter(void* comm, int dtype, void* buf, int64_t count, void* stream);
int mm_comm_all_gather(void* comm, int dtype, void* buf, int64_t count, void* stream);
int mm_comm_finalize(void* comm);

/* AdamW with the fp32 master weight held as (bf16 parameter, int16 remainder): master_bits = (p_bits << 16) + lo, p = RNE(master).
 * Same update as mm_adamw_step (MM_BF16), 26 B instead of 28 B of HBM traffic per parameter and no separate fp32 copy; one
 * remainder value in 2^17 (+0x8000, a round-to-even tie) is stored as 0x7FFF, i.e. the master moves by one fp32 ulp there.
 * mm_master_split / mm_master_join convert between that form and an fp32 master (optimiser checkpoints keep fp32).
 * Contract: d = master_bits - (p_bits << 16) lies in [-0x8000, 0x8000]; lo = min(d, 0x7FFF).  d = +0x8000 happens exactly when
 * the low half is 0x8000 under an even upper half (the tie that rounds down); join(split(w)) is then one fp32 ulp below w, and
 * equals w bit for bit everywhere else -- denormals, a mantissa carry into the exponent, values that round to bf16 infinity
 * and infinity itself included (a NaN may come back quieted).  join is plain integer arithmetic on any (p, lo).
 * mm_adamw_step_split: m, v 16-byte aligned, p, g and lo 8-byte aligned (MM_ERR_ALIGN); otherwise mm_adamw_step's rules.
 * mm_master_split / mm_master_join: n < 0 or, for n > 0, a NULL pointer is MM_ERR_ARG; no alignment rule.                       */
int mm_adamw_step_split(void* p_bf16, const void* g_bf16, void* lo_i16, float* m, float* v, int64_t n, float lr, float beta1,
                        float beta2, float eps, float weight_decay, int step, const float* clip, void* stream);
int mm_master_split(const float* master, int64_t n, void* p_bf16, void* lo_i16, void* stream);
int mm_master_join(const void* p_bf16, const void* lo_i16, int64_t n, float* master, void* stream);

/* ---- image preprocessing on the device (optional row) ---------------------------------------------------
 * Replaces the CPU image processor the reference runs in its collator (image_modality.py:77,88-93 -> HF CLIPImageProcessor:
 * PIL resize BICUBIC, center crop, rescale 1/255, normalize) for an already decoded uint8 RGB image [src_h, src_w, 3] in HBM.
 * Pillow's two-pass fixed-point resampling, bit for bit; the int32 weight tables (bounds [n][2] = first tap, tap count; coef
 * [n][k]) are made on the host exactly as Pillow's precompute_coeffs / normalize_coeffs_8bpc do (dataset/gpu_image.py).
 * mm_image_resample_h: tmp [nrows, cw, 3] uint8 = horizontal pass of source rows r0 .. r0+nrows-1, resized columns left ..
 * left+cw-1.  mm_image_resample_v_norm: out [3, ch, cw] fp32 = vertical pass of resized rows top .. top+ch-1 over tmp, then
 * x * rescale, (x - mean) / std as separate float32 operations (the CPU path's); mean / std are HOST arrays of 3 floats.   */
int mm_image_resample_h(const void* src_u8, int src_h, int src_w, int src_row_stride, int r0, int nrows, const int* xbounds,
                        const int* xcoef, int kx, int left, int cw, void* tmp_u8, void* stream);
int mm_image_resample_v_norm(const void* tmp_u8, int r0, int nrows, int cw, const int* ybounds, const int* ycoef, int ky, int top,
                             int ch, float rescale, int do_rescale, const float* mean3_host, const float* std3_host, int do_norm,
                             float* out_chw, void* stream);

/* ---- utilities ---------------------------------------------------------------------------------------------------- */
int mm_cast(int src_dtype, int dst_dtype, const void* src, void* dst, int64_t n, void* stream);
int mm_fill_zero(void* p, int64_t bytes, void* stream);
int mm_device_cu_count(void);                        /* compute units of the current device (-1: no device) */

/* ---- diagnostics (tests only): raw lane maps of ds_read_b64_tr_b16 and the bf16 MFMAs ------------------------------
 * tr_read: img = 4096 bf16 copied to LDS; lane l reads at byte address addr[l]; out[l*4+j] = its j-th element.
 * mfma: shape 32 -> v_mfma_f32_32x32x16_bf16 (out 64x16 f32), 16 -> v_mfma_f32_16x16x32_bf16 (out 64x4 f32);
 *       a/b = 64 lanes x 8 bf16 fragments.                                                                         */
int mm_debug_tr_read(const void* img_bf16_4096, const void* lane_byte_addr_i32_64, void* out_bf16_256, void* stream);
int mm_debug_mfma(int shape, const void* a_frag_bf16_512, const void* b_frag_bf16_512, void* out_f32, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MM_HIP_H */
