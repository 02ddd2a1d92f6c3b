// Beam search selection on the device: generate(num_beams=n).  The contract (rules a-g, the state layout, the order of ties) is
// written out in include/mm_hip.h (mm_beam_step); tests/beam_ref.py restates it in fp64.
//
// One step is three launches, handed over at launch boundaries only (no arrival counters, no float atomics: fixed reduction
// orders, the same bits on every launch):
//   beam_part_kernel    rows x ceil(V / 4096) workgroups, one thread per 16 contiguous logits (mm_sample's cut): the chunk's
//                       maximum, its sum of exp(x - max) and its K = 2n largest logits in descending order as 64-bit keys
//                       (order-preserving key of x | ~token: a larger key is a larger logit, then the smaller token), by K rounds
//                       of a block-wide maximum
//   beam_merge_kernel   one workgroup per prompt: log-sum-exp of every row (chunks in chunk order), then K rounds over the heads
//                       of the rows x chunks sorted lists give the prompt's K candidates in the contract's order; thread 0 applies
//                       rules c-f on them in LDS; all threads then write the running beams, the hypotheses that finished, and the
//                       new ancestor table
//   beam_done_kernel    rule g over the prompts
// mm_beam_finish ranks every prompt's finished set and gathers the returned ids.
#include "mm_common.h"

#include <math.h>

namespace {

constexpr int BCHUNK = 4096;               // vocabulary entries per workgroup
constexpr int BPT = BCHUNK / 256;          // 16 contiguous entries per thread
constexpr int MAXN = 16;                   // beams per prompt
constexpr int MAXK = 2 * MAXN;             // candidates per prompt
constexpr int MAXV = 1 << 24;
typedef unsigned long long u64;

// order-preserving key: larger x <=> larger key (after -0 -> +0); never 0 for a number
__device__ __forceinline__ unsigned fkey(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float kfloat(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

struct BState {              // the fields of the caller's state buffer (mm_beam_state_layout)
  float* score;              // [R] running scores
  int* parent;               // [R] parents of the last step (relative to the prompt's first row)
  int* tok;                  // [T, R] token chosen at step t for physical row r
  int* anc;                  // [2, T, R] ancestor tables (ping-pong)
  float* fscore;             // [R] finished set: normalised score per slot
  int* flen;                 // [R] length (0: the slot is empty)
  int* fseqno;               // [R] insertion number (ties: the earlier entry wins)
  int* fseq;                 // [R, T] tokens
  int* open;                 // [B]
  int* fcount;               // [B] insertions so far; min(fcount, n) slots are valid
  int* done;                 // [1]
};

struct BArgs {
  const void* logits;
  int B, n, V, ld, C, K, vec;
  int step, T, es;
  int64_t eos;
  float d_i, d_L;            // (step + 1) ** length_penalty, L ** length_penalty
  float* cmax;               // [rows, C]
  float* csum;               // [rows, C]
  u64* ckey;                 // [rows, C, K]
  BState st;
  int64_t* next_ids;         // [R]
};

// block-wide maximum of a 64-bit key over 256 threads; buf = 4 keys of LDS that no earlier use still reads
__device__ __forceinline__ u64 block_max_u64(u64 k, u64* buf) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(k >> 32), o, 64), lo = (unsigned)__shfl_xor((int)(unsigned)k, o, 64);
    const u64 other = ((u64)hi << 32) | lo;
    k = other > k ? other : k;
  }
  if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = k;
  __syncthreads();
  const u64 a = buf[0] > buf[1] ? buf[0] : buf[1], b = buf[2] > buf[3] ? buf[2] : buf[3];
  return a > b ? a : b;
}

template <typename T>
__global__ __launch_bounds__(256) void beam_part_kernel(BArgs a) {
  __shared__ float red[4];
  __shared__ u64 kbuf[2][4];
  const int c = blockIdx.x, r = blockIdx.y;
  const T* row = (const T*)a.logits + (int64_t)r * a.ld;
  const int e0 = c * BCHUNK + (int)threadIdx.x * BPT;
  const int nv = min(BPT, a.V - e0);                       // <= 0: this thread has no entry; columns [V, ld) are never read
  float x[BPT];
  if (a.vec && nv == BPT) {
    constexpr int N = Vec16<T>::N;
    const Vec16<T>* p = (const Vec16<T>*)(row + e0);
#pragma unroll
    for (int i = 0; i < BPT / N; ++i) {
      const Vec16<T> v = p[i];
#pragma unroll
      for (int j = 0; j < N; ++j) x[i * N + j] = v.get(j);
    }
  } else {
#pragma unroll
    for (int j = 0; j < BPT; ++j) x[j] = j < nv ? to_f32(row[e0 + j]) : -INFINITY;
  }
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < BPT; ++j) {
    if (x[j] == 0.f) x[j] = 0.f;                           // -0 -> +0
    if (j < nv) mx = fmaxf(mx, x[j]);
  }
  mx = block_max_256(mx, red);
  float sm = 0.f;
#pragma unroll
  for (int j = 0; j < BPT; ++j)
    if (j < nv && x[j] > -INFINITY) sm += expf(x[j] - mx);
  sm = block_sum_256(sm, red);
  if (threadIdx.x == 0) {
    a.cmax[(int64_t)r * a.C + c] = mx;
    a.csum[(int64_t)r * a.C + c] = sm;
  }
  u64 key[BPT];
#pragma unroll
  for (int j = 0; j < BPT; ++j) key[j] = j < nv ? (((u64)fkey(x[j]) << 32) | (u64)(0xFFFFFFFFu - (unsigned)(e0 + j))) : 0ull;
  u64* out = a.ckey + ((int64_t)r * a.C + c) * a.K;
  for (int k = 0; k < a.K; ++k) {
    u64 best = 0ull;
#pragma unroll
    for (int j = 0; j < BPT; ++j) best = key[j] > best ? key[j] : best;
    const u64 win = block_max_u64(best, kbuf[k & 1]);      // two buffers: round k + 1 writes the other one, one barrier per round
#pragma unroll
    for (int j = 0; j < BPT; ++j)
      if (key[j] == win) key[j] = 0ull;                    // keys are unique (the token is part of them); 0: the chunk has run out
    if (threadIdx.x == 0) out[k] = win;
  }
}

// a candidate in the contract's order: larger lp, then the smaller row, then the larger logit, then the smaller token
struct Cand {
  unsigned lpk, rowk;        // fkey(lp), MAXN - 1 - j
  u64 key;                   // the chunk list's key
};
__device__ __forceinline__ bool cand_gt(const Cand& p, const Cand& q) {
  if (p.lpk != q.lpk) return p.lpk > q.lpk;
  if (p.rowk != q.rowk) return p.rowk > q.rowk;
  return p.key > q.key;
}
__device__ __forceinline__ Cand cand_shfl(const Cand& p, int o) {
  Cand q;
  q.lpk = (unsigned)__shfl_xor((int)p.lpk, o, 64);
  q.rowk = (unsigned)__shfl_xor((int)p.rowk, o, 64);
  q.key = ((u64)(unsigned)__shfl_xor((int)(unsigned)(p.key >> 32), o, 64) << 32) | (unsigned)__shfl_xor((int)(unsigned)p.key, o, 64);
  return q;
}

__global__ __launch_bounds__(256) void beam_merge_kernel(BArgs a) {
  __shared__ float lse[MAXN], sc[MAXN];
  __shared__ Cand wbuf[2][4];
  __shared__ float c_lp[MAXK];
  __shared__ int c_j[MAXK], c_v[MAXK];
  __shared__ float f_score[MAXN];
  __shared__ int f_len[MAXN], f_seqno[MAXN];
  __shared__ float n_s[MAXN];
  __shared__ int n_par[MAXN], n_tok[MAXN];
  __shared__ int ins_slot[MAXN], ins_rank[MAXN];
  __shared__ int n_ins;
  const int b = blockIdx.x, tid = threadIdx.x, n = a.n, K = a.K, C = a.C, step = a.step;
  const int R = a.B * n;
  const int nrows = step == 0 ? 1 : n;                                   // step 0: the prefill's one row per prompt
  const int64_t row0 = step == 0 ? b : (int64_t)b * n;
  const int base = b * n;                                                // the prompt's first beam row
  if (tid < nrows) {
    const float* cm = a.cmax + (row0 + tid) * C;
    const float* cs = a.csum + (row0 + tid) * C;
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, cm[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c)
      if (cm[c] > -INFINITY) s += cs[c] * expf(cm[c] - m);               // chunk order
    lse[tid] = m + logf(s);
    sc[tid] = step == 0 ? 0.f : a.st.score[base + tid];
  }
  if (tid < n) {
    const bool init = step == 0;                                         // step 0 starts the prompt's state
    f_score[tid] = init ? -INFINITY : a.st.fscore[base + tid];
    f_len[tid] = init ? 0 : a.st.flen[base + tid];
    f_seqno[tid] = init ? 0 : a.st.fseqno[base + tid];
  }
  __syncthreads();
  // K rounds over the heads of the nrows * C sorted lists; list q = j C + c belongs to thread q % 256, which is the only one that
  // reads it and marks a taken entry by writing 0 over it (the taken entries of a list are a prefix of it)
  const int nlists = nrows * C;
  for (int k = 0; k < K; ++k) {
    Cand best{0u, 0u, 0ull};
    u64* best_at = nullptr;
    for (int q = tid; q < nlists; q += 256) {
      const int j = q / C;
      u64* lst = a.ckey + (row0 * C + q) * K;
      for (int e = 0; e < K; ++e) {
        const u64 key = lst[e];
        if (key == 0ull) continue;                                       // taken, or past the end of a short chunk
        float lp = sc[j] + (kfloat((unsigned)(key >> 32)) - lse[j]);
        if (!(lp > -INFINITY)) lp = -INFINITY;                           // NaN (a row without a finite logit) ranks last
        if (lp == 0.f) lp = 0.f;
        const Cand cnd{fkey(lp), (unsigned)(MAXN - 1 - j), key};
        if (cand_gt(cnd, best)) { best = cnd; best_at = lst + e; }
        break;                                                           // the head of this list
      }
    }
    Cand w = best;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const Cand other = cand_shfl(w, o);
      if (cand_gt(other, w)) w = other;
    }
    Cand* buf = wbuf[k & 1];
    if ((tid & 63) == 0) buf[tid >> 6] = w;
    __syncthreads();
    Cand win = buf[0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
      if (cand_gt(buf[i], win)) win = buf[i];
    const bool none = win.key == 0ull;
    if (!none && best_at && best.key == win.key && best.rowk == win.rowk) *best_at = 0ull;      // (row, token) is unique
    if (tid == 0) {
      c_lp[k] = none ? -INFINITY : kfloat(win.lpk);
      c_j[k] = none ? 0 : MAXN - 1 - (int)win.rowk;
      c_v[k] = none ? -1 : (int)(0xFFFFFFFFu - (unsigned)win.key);
    }
  }
  __syncthreads();
  if (tid == 0) {
    const bool last = step + 1 == a.T;
    int open = step == 0 ? 1 : (a.st.open[b] != 0);
    int fcount = step == 0 ? 0 : a.st.fcount[b];
    const bool full_before = fcount >= n;
    // d: the next running beams
    int nrun = 0;
    for (int c = 0; c < K && nrun < n; ++c) {
      const bool live = c_v[c] >= 0 && c_lp[c] > -INFINITY;
      if (live && !(last || (int64_t)c_v[c] == a.eos)) { n_par[nrun] = c_j[c]; n_tok[nrun] = c_v[c]; n_s[nrun] = c_lp[c]; ++nrun; }
    }
    const bool has_run = nrun > 0;
    for (int r = nrun; r < n; ++r) { n_par[r] = r; n_tok[r] = (int)a.eos; n_s[r] = -INFINITY; }       // not used again (last step)
    // e: the finished set
    int ni = 0;
    if (open && !(a.es == 1 && full_before)) {
      for (int c = 0; c < n; ++c) {
        const bool live = c_v[c] >= 0 && c_lp[c] > -INFINITY;
        if (!live || !(last || (int64_t)c_v[c] == a.eos)) continue;
        const float sv = c_lp[c] / a.d_i;
        int slot = -1;
        if (fcount < n) {
          for (int i = 0; i < n && slot < 0; ++i)
            if (f_len[i] == 0) slot = i;
        } else {
          int wst = 0;                                                   // the worst entry: lowest score, then the latest insertion
          for (int i = 1; i < n; ++i)
            if (f_score[i] < f_score[wst] || (f_score[i] == f_score[wst] && f_seqno[i] > f_seqno[wst])) wst = i;
          if (sv > f_score[wst]) slot = wst;                             // on a tie the existing entry stays
        }
        if (slot < 0) continue;
        f_score[slot] = sv;
        f_len[slot] = step + 1;
        f_seqno[slot] = fcount++;
        ins_slot[ni] = slot;
        ins_rank[ni] = c;
        ++ni;
      }
    }
    n_ins = ni;
    // f
    if (fcount >= n) {
      float worst = f_score[0];
      for (int i = 1; i < n; ++i) worst = fminf(worst, f_score[i]);
      const float s0 = has_run ? n_s[0] / a.d_L : -INFINITY;
      open = open && (s0 > worst);
    }
    a.st.open[b] = open;
    a.st.fcount[b] = fcount;
  }
  __syncthreads();
  const int* anc_old = a.st.anc + (int64_t)(step & 1) * a.T * R;
  int* anc_new = a.st.anc + (int64_t)((step + 1) & 1) * a.T * R;
  auto clampr = [&](int p) { return p < base ? base : (p > base + n - 1 ? base + n - 1 : p); };
  // hypotheses that entered the finished set: the parent's tokens through the old table, then the candidate's token
  for (int k = 0; k < n_ins; ++k) {
    const int slot = ins_slot[k], c = ins_rank[k];
    int* dst = a.st.fseq + (int64_t)(base + slot) * a.T;
    for (int t = tid; t <= step; t += 256)
      dst[t] = t == step ? c_v[c] : a.st.tok[(int64_t)t * R + clampr(anc_old[(int64_t)t * R + base + c_j[c]])];
  }
  if (tid < n) {
    a.st.fscore[base + tid] = f_score[tid];
    a.st.flen[base + tid] = f_len[tid];
    a.st.fseqno[base + tid] = f_seqno[tid];
    a.st.score[base + tid] = n_s[tid];
    a.st.parent[base + tid] = n_par[tid];
    a.st.tok[(int64_t)step * R + base + tid] = n_tok[tid];
    a.next_ids[base + tid] = (int64_t)n_tok[tid];
    anc_new[(int64_t)step * R + base + tid] = base + tid;               // the slot the coming step appends to
  }
  for (int i = tid; i < step * n; i += 256) {
    const int t = i / n, r = i % n;
    anc_new[(int64_t)t * R + base + r] = clampr(anc_old[(int64_t)t * R + base + n_par[r]]);
  }
}

__global__ void beam_done_kernel(BArgs a) {
  if (threadIdx.x != 0) return;
  bool any_open = false, all_full = true;
  for (int b = 0; b < a.B; ++b) {
    any_open = any_open || a.st.open[b] != 0;
    all_full = all_full && a.st.fcount[b] >= a.n;
  }
  a.st.done[0] = (!any_open || (a.es == 1 && all_full) || a.step + 1 == a.T) ? 1 : 0;
}

__global__ __launch_bounds__(256) void beam_finish_kernel(BState st, int B, int n, int T, int nrs, int64_t eos, int64_t* ids, float* scores,
                                                          int* lens) {
  __shared__ int order[MAXN];
  const int b = blockIdx.x, base = b * n;
  if (threadIdx.x == 0) {
    // rank of slot i = the number of slots before it: valid first, then the higher score, then the earlier insertion
    for (int i = 0; i < n; ++i) order[i] = i;                // a state no step wrote (equal arrivals, NaN) still names slots in range
    for (int i = 0; i < n; ++i) {
      int rank = 0;
      for (int j = 0; j < n; ++j) {
        if (j == i) continue;
        const bool vi = st.flen[base + i] > 0, vj = st.flen[base + j] > 0;
        const float si = st.fscore[base + i], sj = st.fscore[base + j];
        const int qi = st.fseqno[base + i], qj = st.fseqno[base + j];
        bool before;
        if (vi != vj) before = vj;
        else if (!vi) before = j < i;
        else if (sj != si) before = sj > si;
        else if (qj != qi) before = qj < qi;
        else before = j < i;
        rank += before ? 1 : 0;
      }
      order[rank] = i;
    }
  }
  __syncthreads();
  for (int k = 0; k < nrs; ++k) {
    const int slot = order[k], len = min(max(st.flen[base + slot], 0), T);
    const int64_t o = (int64_t)b * nrs + k;
    for (int t = threadIdx.x; t < T; t += 256) ids[o * T + t] = t < len ? (int64_t)st.fseq[(int64_t)(base + slot) * T + t] : eos;
    if (threadIdx.x == 0) {
      scores[o] = len > 0 ? st.fscore[base + slot] : -INFINITY;
      lens[o] = len;
    }
  }
}

constexpr int NFIELDS = 11;
struct StLayout {
  int64_t off[NFIELDS], total;
};
StLayout st_layout(int B, int n, int T) {
  const int64_t R = (int64_t)B * n;
  auto up = [](int64_t b) { return (b + 15) / 16 * 16; };
  const int64_t bytes[NFIELDS] = {R * 4, R * 4, R * T * 4, 2 * R * T * 4, R * 4, R * 4, R * 4, R * T * 4, (int64_t)B * 4, (int64_t)B * 4, 4};
  StLayout L;
  int64_t at = 0;
  for (int i = 0; i < NFIELDS; ++i) { L.off[i] = at; at += up(bytes[i]); }
  L.total = at;
  return L;
}
BState st_fields(void* state, const StLayout& L) {
  char* p = (char*)state;
  return BState{(float*)(p + L.off[0]), (int*)(p + L.off[1]), (int*)(p + L.off[2]), (int*)(p + L.off[3]), (float*)(p + L.off[4]),
                (int*)(p + L.off[5]), (int*)(p + L.off[6]), (int*)(p + L.off[7]), (int*)(p + L.off[8]), (int*)(p + L.off[9]),
                (int*)(p + L.off[10])};
}

struct WsLayout {
  int64_t ckey, cmax, csum, total;
};
WsLayout ws_layout(int B, int n, int V) {
  const int64_t C = (V + BCHUNK - 1) / BCHUNK, R = (int64_t)B * n, K = 2 * n;
  auto up = [](int64_t b) { return (b + 15) / 16 * 16; };
  WsLayout L;
  L.ckey = 0;
  L.cmax = L.ckey + up(R * C * K * 8);
  L.csum = L.cmax + up(R * C * 4);
  L.total = L.csum + up(R * C * 4);
  return L;
}

bool shape_ok(int B, int n, int T) { return B >= 1 && n >= 1 && n <= MAXN && T >= 1 && (int64_t)B * n * T <= 0x7FFFFFFF / 8; }

}  // namespace

extern "C" int mm_beam_ws_bytes(int B, int n, int V, int64_t* bytes) {
  if (!bytes || B < 1 || n < 1 || n > MAXN || V < 2 * n || V > MAXV || (int64_t)B * n > 65535) return MM_ERR_ARG;
  *bytes = ws_layout(B, n, V).total;
  return MM_OK;
}

extern "C" int mm_beam_state_bytes(int B, int n, int max_new_tokens, int64_t* bytes) {
  if (!bytes || !shape_ok(B, n, max_new_tokens)) return MM_ERR_ARG;
  *bytes = st_layout(B, n, max_new_tokens).total;
  return MM_OK;
}

extern "C" int mm_beam_state_layout(int B, int n, int max_new_tokens, int64_t* offsets) {
  if (!offsets || !shape_ok(B, n, max_new_tokens)) return MM_ERR_ARG;
  const StLayout L = st_layout(B, n, max_new_tokens);
  for (int i = 0; i < NFIELDS; ++i) offsets[i] = L.off[i];
  return MM_OK;
}

extern "C" int mm_beam_step(int dtype, const void* logits, int B, int n, int V, int ld, int step, int max_new_tokens, int64_t eos,
                            float length_penalty, int early_stopping, void* state, int64_t state_bytes, void* ws, int64_t ws_bytes,
                            int64_t* next_ids, void* stream) {
  if (dtype != MM_BF16 && dtype != MM_F32) return MM_ERR_ARG;
  if (!logits || !state || !ws || !next_ids) return MM_ERR_ARG;
  if (!shape_ok(B, n, max_new_tokens) || (int64_t)B * n > 65535 || V < 2 * n || V > MAXV || ld < V) return MM_ERR_ARG;
  if (step < 0 || step >= max_new_tokens || early_stopping < 0 || early_stopping > 2 || !isfinite(length_penalty)) return MM_ERR_ARG;
  const StLayout SL = st_layout(B, n, max_new_tokens);
  const WsLayout WL = ws_layout(B, n, V);
  if (state_bytes < SL.total || ws_bytes < WL.total) return MM_ERR_ARG;
  if ((((uintptr_t)ws) & 15) || (((uintptr_t)state) & 15)) return MM_ERR_ALIGN;
  BArgs a;
  a.logits = logits;
  a.B = B;
  a.n = n;
  a.V = V;
  a.ld = ld;
  a.C = (V + BCHUNK - 1) / BCHUNK;
  a.K = 2 * n;
  a.vec = mm_aligned16(logits) && ((int64_t)ld * mm_elem_size(dtype)) % 16 == 0;
  a.step = step;
  a.T = max_new_tokens;
  a.es = early_stopping;
  a.eos = eos;
  const int L = (early_stopping == 2 && length_penalty > 0.f) ? max_new_tokens : step + 1;
  a.d_i = (float)pow((double)(step + 1), (double)length_penalty);
  a.d_L = (float)pow((double)L, (double)length_penalty);
  char* w = (char*)ws;
  a.ckey = (u64*)(w + WL.ckey);
  a.cmax = (float*)(w + WL.cmax);
  a.csum = (float*)(w + WL.csum);
  a.st = st_fields(state, SL);
  a.next_ids = next_ids;
  hipStream_t s = (hipStream_t)stream;
  const int rows = step == 0 ? B : B * n;
  const dim3 grid((unsigned)a.C, (unsigned)rows), block(256);
  if (dtype == MM_BF16)
    hipLaunchKernelGGL(beam_part_kernel<bf16>, grid, block, 0, s, a);
  else
    hipLaunchKernelGGL(beam_part_kernel<float>, grid, block, 0, s, a);
  MM_CHECK_LAUNCH();
  hipLaunchKernelGGL(beam_merge_kernel, dim3((unsigned)B), block, 0, s, a);
  MM_CHECK_LAUNCH();
  hipLaunchKernelGGL(beam_done_kernel, dim3(1), dim3(64), 0, s, a);
  MM_CHECK_LAUNCH();
  return MM_OK;
}

extern "C" int mm_beam_finish(const void* state, int64_t state_bytes, int B, int n, int max_new_tokens, int num_return, int64_t eos,
                              int64_t* ids, float* scores, int32_t* lens, void* stream) {
  if (!state || !ids || !scores || !lens) return MM_ERR_ARG;
  if (!shape_ok(B, n, max_new_tokens) || num_return < 1 || num_return > n) return MM_ERR_ARG;
  const StLayout SL = st_layout(B, n, max_new_tokens);
  if (state_bytes < SL.total) return MM_ERR_ARG;
  if (((uintptr_t)state) & 15) return MM_ERR_ALIGN;
  hipLaunchKernelGGL(beam_finish_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, st_fields((void*)state, SL), B, n,
                     max_new_tokens, num_return, eos, ids, scores, lens);
  MM_CHECK_LAUNCH();
  return MM_OK;
}
