// Prompt-lookup speculative decoding of generate() on the device (prompt_lookup_num_tokens = k): the draft rule of transformers'
// PromptLookupCandidateGenerator.get_candidates per row, the cache append of a verify step's k + 1 positions at per-row slots, and
// the acceptance bookkeeping.  The contracts are written out in include/mm_hip.h (mm_lookup_draft, mm_kv_append_at,
// mm_lookup_accept); tests/lookup_ref.py restates the two rules in Python.  The decode attention of the verify step is
// mm_attn_decode_verify (mm_attn.hip).
//
// Nothing here is on the bandwidth path: a draft scans at most max_ngram * L int32 ids of one row (L2-resident), the append copies
// B (k + 1) 2 Hkv D bf16, the accept touches 16 rows.  They exist so that the loop never brings a token to the host.
#include "mm_common.h"

namespace {

constexpr int LK_ROWS_MAX = 16;      // rows of a verify step: B (k + 1) <= 16 activation rows of the streaming linears

struct DraftArgs {
  const int32_t *hist, *hlen, *count, *finished, *base;
  int ld_hist, k, max_ngram, max_new;
  int64_t eos;
  int64_t *ids, *pos;
  int32_t* n_draft;
};

// One workgroup per row.  For g = min(G, L - 1) .. 1 every thread compares the windows i = tid, tid + 256, .. < L - g with the tail
// and the workgroup takes the smallest matching i (integer LDS atomicMin: order-free); the first g with a match decides.
__global__ __launch_bounds__(256) void lookup_draft_kernel(DraftArgs a) {
  __shared__ int first;
  const int r = blockIdx.x, tid = threadIdx.x;
  const int32_t* h = a.hist + (int64_t)r * a.ld_hist;
  const int L = min(max(a.hlen[r], 0), a.ld_hist);
  const int Q = a.k + 1;
  const bool active = a.finished[r] == 0 && a.count[r] < a.max_new;
  int start = -1;
  if (active) {                                   // workgroup-uniform
    for (int g = min(a.max_ngram, L - 1); g >= 1; --g) {
      if (tid == 0) first = 0x7FFFFFFF;
      __syncthreads();
      const int32_t* tail = h + (L - g);
      int mine = 0x7FFFFFFF;
      for (int i = tid; i < L - g; i += 256) {
        bool same = true;
        for (int u = 0; u < g && same; ++u) same = h[i + u] == tail[u];
        if (same) { mine = i; break; }           // ascending per thread: its first match is its smallest
      }
      if (mine != 0x7FFFFFFF) atomicMin(&first, mine);
      __syncthreads();
      const int f = first;
      __syncthreads();                            // every thread has read `first` before the next g resets it
      if (f != 0x7FFFFFFF) { start = f + g; break; }
    }
  }
  if (tid == 0) {
    const int64_t last = L > 0 ? (int64_t)h[L - 1] : 0;
    int n = 0;
    int64_t* ids = a.ids + (int64_t)r * Q;
    int64_t* pos = a.pos + (int64_t)r * Q;
    ids[0] = last;
    if (start >= 0) {
      const int room = a.max_new - a.count[r] - 1;
      const int end = min(start + a.k, L);
      while (start + n < end && n < room && (int64_t)h[start + n] != a.eos) {
        ids[1 + n] = (int64_t)h[start + n];
        ++n;
      }
    }
    for (int j = 1 + n; j < Q; ++j) ids[j] = last;
    const int64_t b0 = a.base[r];
    for (int j = 0; j < Q; ++j) pos[j] = b0 + j;
    a.n_draft[r] = n;
  }
}

struct AppendArgs {
  const bf16* x;
  int ld, Q, Hq, Hkv, D, Smax;
  const int32_t* base;
  bf16 *kc, *vc;
  int64_t c_sb, c_ss;
};

// One workgroup per (row b Q + j): 16-byte copies of the row's Hkv D k elements and Hkv D v elements.
__global__ __launch_bounds__(256) void kv_append_at_kernel(AppendArgs a) {
  const int row = blockIdx.x, b = row / a.Q, j = row % a.Q;
  const int64_t slot = (int64_t)a.base[b] + j;
  if (slot < 0 || slot >= a.Smax) return;         // workgroup-uniform: nothing is written for a slot outside the cache
  const int nkv = a.Hkv * a.D;                    // elements of the row's k (and of its v); the cache's heads are contiguous
  const bf16* xk = a.x + (int64_t)row * a.ld + (int64_t)a.Hq * a.D;
  const bf16* xv = xk + nkv;
  bf16* kd = a.kc + b * a.c_sb + slot * a.c_ss;
  bf16* vd = a.vc + b * a.c_sb + slot * a.c_ss;
  for (int e = threadIdx.x * 8; e < nkv; e += 256 * 8) {
    *(bf16x8*)(kd + e) = *(const bf16x8*)(xk + e);
    *(bf16x8*)(vd + e) = *(const bf16x8*)(xv + e);
  }
}

struct AcceptArgs {
  const int64_t *tok, *ids;
  const int32_t* n_draft;
  int rows, Q, max_new, ld_out, ld_hist;
  int64_t eos;
  int64_t* out;
  int32_t *hist, *hlen, *count, *finished, *base, *stats, *done;
};

// One workgroup of 64 threads; thread r owns row r (at most Q = 16 ids per row).
__global__ __launch_bounds__(64) void lookup_accept_kernel(AcceptArgs a) {
  __shared__ int live[LK_ROWS_MAX];
  const int r = threadIdx.x;
  if (r < a.rows) {
    int cnt = a.count[r], fin = a.finished[r];
    if (fin == 0 && cnt < a.max_new) {
      const int64_t* tok = a.tok + (int64_t)r * a.Q;
      int nd = 0;
      if (a.Q > 1) nd = min(max(a.n_draft[r], 0), a.Q - 1);
      int acc = 0;
      while (acc < nd && a.ids[(int64_t)r * a.Q + 1 + acc] == tok[acc]) ++acc;
      const int hl = a.hlen[r];
      int m = 0;
      for (int j = 0; j <= acc && cnt < a.max_new && !fin; ++j) {
        const int64_t t = tok[j];
        a.out[(int64_t)r * a.ld_out + cnt] = t;           // cnt < max_new <= ld_out
        if (hl + m >= 0 && hl + m < a.ld_hist) a.hist[(int64_t)r * a.ld_hist + hl + m] = (int32_t)t;
        ++cnt;
        ++m;
        if (t == a.eos) fin = 1;
      }
      a.count[r] = cnt;
      a.hlen[r] = hl + m;
      a.base[r] += m;
      a.finished[r] = fin;
      a.stats[2 * r] += 1;
      a.stats[2 * r + 1] += m - 1;
    }
    live[r] = fin == 0 && cnt < a.max_new;
  }
  __syncthreads();
  if (r == 0) {
    int any = 0;
    for (int i = 0; i < a.rows; ++i) any |= live[i];
    a.done[0] = any ? 0 : 1;
  }
}

}  // namespace

extern "C" int mm_lookup_draft(const int32_t* hist, int ld_hist, const int32_t* hlen, const int32_t* count, const int32_t* finished,
                               const int32_t* base, int rows, int k, int max_ngram, int max_new, int64_t eos, int64_t* ids,
                               int64_t* pos, int32_t* n_draft, void* stream) {
  if (!hist || !hlen || !count || !finished || !base || !ids || !pos || !n_draft) return MM_ERR_ARG;
  if (rows < 0 || rows > LK_ROWS_MAX || k < 1 || k > 15 || max_ngram < 1 || max_new < 1 || ld_hist < 1) return MM_ERR_ARG;
  if (rows == 0) return MM_OK;
  DraftArgs a{hist, hlen, count, finished, base, ld_hist, k, max_ngram, max_new, eos, ids, pos, n_draft};
  hipLaunchKernelGGL(lookup_draft_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, a);
  MM_CHECK_LAUNCH();
  return MM_OK;
}

extern "C" int mm_kv_append_at(int dtype, const void* x, int ld, int B, int Q, int Hq, int Hkv, int D, const int32_t* base,
                               void* kcache, void* vcache, int64_t c_sb, int64_t c_ss, int Smax, void* stream) {
  if (!x || !base || !kcache || !vcache) return MM_ERR_ARG;
  if (B < 0 || Q < 1 || Q > 16 || Hq < 1 || Hkv < 1 || D < 1 || Smax < 1) return MM_ERR_ARG;
  if ((int64_t)ld < ((int64_t)Hq + 2 * (int64_t)Hkv) * D || (int64_t)B * Q > 0x7FFFFFFF) return MM_ERR_ARG;
  if (c_ss < (int64_t)Hkv * D || (B > 1 && c_sb < (int64_t)Smax * c_ss)) return MM_ERR_ARG;      // slots and sequences do not overlap
  if (dtype != MM_BF16 || D % 8) return MM_ERR_UNSUPPORTED;
  if ((ld & 7) || (c_sb & 7) || (c_ss & 7)) return MM_ERR_ALIGN;
  if (!mm_aligned16(x) || !mm_aligned16(kcache) || !mm_aligned16(vcache)) return MM_ERR_ALIGN;
  if (B == 0) return MM_OK;
  AppendArgs a{(const bf16*)x, ld, Q, Hq, Hkv, D, Smax, base, (bf16*)kcache, (bf16*)vcache, c_sb, c_ss};
  hipLaunchKernelGGL(kv_append_at_kernel, dim3(B * Q), dim3(256), 0, (hipStream_t)stream, a);
  MM_CHECK_LAUNCH();
  return MM_OK;
}

extern "C" int mm_lookup_accept(const int64_t* tok, const int64_t* ids, const int32_t* n_draft, int rows, int Q, int max_new,
                                int64_t eos, int64_t* out, int ld_out, int32_t* hist, int ld_hist, int32_t* hlen, int32_t* count,
                                int32_t* finished, int32_t* base, int32_t* stats, int32_t* done, void* stream) {
  if (!tok || !out || !hist || !hlen || !count || !finished || !base || !stats || !done) return MM_ERR_ARG;
  if (rows < 0 || rows > LK_ROWS_MAX || Q < 1 || Q > 16 || max_new < 1 || ld_out < max_new || ld_hist < 1) return MM_ERR_ARG;
  if (Q > 1 && (!ids || !n_draft)) return MM_ERR_ARG;
  if (rows == 0) return MM_OK;
  AcceptArgs a{tok, ids, n_draft, rows, Q, max_new, ld_out, ld_hist, eos, out, hist, hlen, count, finished, base, stats, done};
  hipLaunchKernelGGL(lookup_accept_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
  MM_CHECK_LAUNCH();
  return MM_OK;
}
