// CTC negative log likelihood over the Listener's frames: the auxiliary branch of BASELINE.json
// configs[3] ("Joint CTC+attention loss").  BUILD-DEFINED: the reference has no CTC anywhere
// (src/trainer.py:426-434 is its only loss), so there is no reference line to
// follow; the semantics are those of torch.nn.functional.ctc_loss(log_softmax(logits), labels,
// frame_lens, label_lens, blank, reduction='mean', zero_infinity=True), which tests/ use as the checker.
//
// One workgroup per utterance.  The utterance's log-probability table [len][V] lives in LDS
// (75 KB at T' = 375, V = 50), the lattice row alpha_t / beta_t in a double-buffered LDS line, so a
// step of the recursion is LDS reads, three exp and one log per state, and one barrier.  The alpha
// lattice goes to HBM once (fire-and-forget stores) and is read back once by the backward kernel,
// one step ahead of its use.  HBM-bound work in principle, latency-bound in practice: len dependent
// steps of about half a microsecond each.
//
// Precision: lattice values are log-probabilities of magnitude ~ nll (hundreds), where a float
// carries 3e-5; summed over len steps that costs 2e-4 of relative error in the posteriors.  The
// lattice is therefore held in double, while every exp / log runs in float on DIFFERENCES from the
// running maximum (magnitude <= log 3 on the way out), which is where a float is exact enough.
#include "../../include/ssasr.h"
#include "common.h"
#include "ctc_prefix.h"

#include <cmath>

namespace {

// One lattice state (and one class) per thread -- the step is a latency chain, so states are spread
// over as many waves as it takes and no wider: 256, 512 or 1024 threads by 2 * Lmax + 1 and V.
constexpr int CTC_MAX_PER_THREAD = 1;
constexpr int CTC_MAX_STATES = 1024;
constexpr int64_t CTC_LDS_TABLE_BYTES = 128 * 1024;         // larger tables stay in the workspace

struct CtcArgs {
  const float* logits;       // [B][T][V]
  const int32_t* frame_lens; // [B]
  const int32_t* y;          // label j of row b: y[b * y_ld + j]
  int64_t y_ld;
  const int32_t* label_lens; // [B]
  int T, V, Sp, blank;       // Sp = 2 * Lmax + 1: row length of the stored lattice
  double* alpha;             // [B][T][Sp]
  double* nll;               // [B]  (+inf: no alignment exists)
  float* table;              // [B][T][V] or nullptr when the table fits LDS
  const float* dloss;        // backward only
  float* dlogits;            // backward only, [B][T][V]
  float* dbias;              // backward only, optional [V], accumulated
  int B;
};

constexpr double NEG_INF = -INFINITY;

// v_exp_f32 / v_log_f32 (about 1 ulp): arguments here are differences <= 0 from a running maximum and
// sums in [1, 3], so the absolute error stays near 1e-7 -- the library calls cost 3x the step time
__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(1.4426950408889634f * x); }
__device__ __forceinline__ float fast_log(float x) { return 0.6931471805599453f * __builtin_amdgcn_logf(x); }

__device__ __forceinline__ double lse3(double a, double b, double c) {
  const double m = fmax(a, fmax(b, c));
  if (m == NEG_INF) return NEG_INF;
  return m + (double)fast_log(fast_exp((float)(a - m)) + fast_exp((float)(b - m)) + fast_exp((float)(c - m)));
}

// log_softmax of the utterance's first `len` rows into `lp` (LDS or workspace): a coalesced copy,
// then one wave per row.
template <int NT>
__device__ void ctc_table(const float* logits, float* lp, int len, int V) {
  const int n = len * V;
  for (int i = threadIdx.x; i < n; i += NT) lp[i] = logits[i];
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int t = wave; t < len; t += NT / 64) {
    float* row = lp + (int64_t)t * V;
    float m = -INFINITY;
    for (int v = lane; v < V; v += 64) m = fmaxf(m, row[v]);
    m = wave_max(m);
    float s = 0.f;
    for (int v = lane; v < V; v += 64) s += expf(row[v] - m);
    s = wave_sum(s);
    const double l = (double)m + (double)logf(s);
    for (int v = lane; v < V; v += 64) row[v] = (float)((double)row[v] - l);
  }
  __syncthreads();
}

// Extended label sequence in LDS: sl[s] = blank for even s, label (s - 1) / 2 for odd s.
template <int NT>
__device__ void ctc_labels(const CtcArgs& a, int b, int L, int* sl) {
  const int S = 2 * L + 1;
  const int32_t* yr = a.y + (int64_t)b * a.y_ld;
  for (int s = threadIdx.x; s < S; s += NT) sl[s] = (s & 1) ? yr[s >> 1] : a.blank;
}

// LDS of both kernels: two lattice lines of Sp + 2 doubles, Sp extended labels, [2][V] class sums
// (backward only), then the table.
__device__ __forceinline__ int ctc_line_doubles(int Sp) { return Sp + 2; }

template <bool LDS_TABLE, int NT>
__global__ __launch_bounds__(NT) void ctc_alpha_kernel(CtcArgs a) {
  extern __shared__ double smem_d[];
  const int b = blockIdx.x;
  const int len = min(a.frame_lens[b], a.T), L = a.label_lens[b], S = 2 * L + 1, V = a.V;
  double* line0 = smem_d;                    // [2 pads][Sp]
  double* line1 = line0 + ctc_line_doubles(a.Sp);
  int* sl = reinterpret_cast<int*>(line1 + ctc_line_doubles(a.Sp));
  float* lp = LDS_TABLE ? reinterpret_cast<float*>(sl + a.Sp) : a.table + (int64_t)b * a.T * V;
  if (len < 1 || L < 0 || S > a.Sp) {        // nothing to align
    if (threadIdx.x == 0) a.nll[b] = INFINITY;
    return;
  }
  ctc_labels<NT>(a, b, L, sl);
  ctc_table<NT>(a.logits + (int64_t)b * a.T * V, lp, len, V);   // (its barriers also publish sl)

  int lab[CTC_MAX_PER_THREAD];
  bool skip[CTC_MAX_PER_THREAD];
#pragma unroll
  for (int k = 0; k < CTC_MAX_PER_THREAD; ++k) {
    const int s = threadIdx.x + k * NT;
    lab[k] = s < S ? sl[s] : a.blank;
    skip[k] = s < S && (s & 1) && s >= 3 && sl[s] != sl[s - 2];
  }
  if (threadIdx.x < 2) { line0[threadIdx.x] = NEG_INF; line1[threadIdx.x] = NEG_INF; }
  double* alpha = a.alpha + (int64_t)b * a.T * a.Sp;
#pragma unroll
  for (int k = 0; k < CTC_MAX_PER_THREAD; ++k) {
    const int s = threadIdx.x + k * NT;
    if (s < S) {
      const double v = s < 2 ? (double)lp[lab[k]] : NEG_INF;
      line0[2 + s] = v;
      alpha[s] = v;
    }
  }
  __syncthreads();
  double* prev = line0;
  double* cur = line1;
  for (int t = 1; t < len; ++t) {
    const float* row = lp + (int64_t)t * V;
#pragma unroll
    for (int k = 0; k < CTC_MAX_PER_THREAD; ++k) {
      const int s = threadIdx.x + k * NT;
      if (s < S) {
        const double v = lse3(prev[2 + s], prev[1 + s], skip[k] ? prev[s] : NEG_INF) + (double)row[lab[k]];
        cur[2 + s] = v;
        alpha[(int64_t)t * a.Sp + s] = v;
      }
    }
    __syncthreads();
    double* tmp = prev; prev = cur; cur = tmp;
  }
  if (threadIdx.x == 0) {
    const double tail = lse3(prev[2 + S - 1], S > 1 ? prev[2 + S - 2] : NEG_INF, NEG_INF);
    a.nll[b] = -tail;                        // +inf when no alignment fits len frames
  }
}

// loss = mean_b( nll_b / max(L_b, 1) ), rows without an alignment counted as 0 (zero_infinity)
__global__ void ctc_mean_kernel(const double* nll, const int32_t* label_lens, int B, float* loss) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) {
      const double v = nll[b];
      if (v < (double)INFINITY) s += v / (double)max(label_lens[b], 1);
    }
    *loss = (float)(s / (double)B);
  }
}

// d loss / d logits[b][t][v] = scale_b * ( softmax[t][v] - sum_{s: label(s) = v} exp(alpha_t(s) + beta_t(s) + nll - lp[t][v]) )
// with scale_b = dloss / (B * max(L_b, 1)); zero for frames past the utterance and for rows without
// an alignment.  One barrier per step: the per-class sums alternate between two LDS rows.
template <bool LDS_TABLE, int NT>
__global__ __launch_bounds__(NT) void ctc_beta_kernel(CtcArgs a) {
  extern __shared__ double smem_d[];
  const int b = blockIdx.x;
  const int len = min(a.frame_lens[b], a.T), L = a.label_lens[b], S = 2 * L + 1, V = a.V;
  double* line0 = smem_d;                    // [Sp][2 pads]
  double* line1 = line0 + ctc_line_doubles(a.Sp);
  int* sl = reinterpret_cast<int*>(line1 + ctc_line_doubles(a.Sp));
  float* acc = reinterpret_cast<float*>(sl + a.Sp);          // [2][V]
  float* lp = LDS_TABLE ? acc + 2 * V : a.table + (int64_t)b * a.T * V;
  float* dl = a.dlogits + (int64_t)b * a.T * V;
  const double nll = a.nll[b];
  const bool feasible = len >= 1 && L >= 0 && S <= a.Sp && nll < (double)INFINITY;
  const int live = feasible ? len : 0;
  for (int i = live * V + threadIdx.x; i < a.T * V; i += NT) dl[i] = 0.f;
  if (!feasible) return;
  ctc_labels<NT>(a, b, L, sl);
  ctc_table<NT>(a.logits + (int64_t)b * a.T * V, lp, len, V);
  const float scale = *a.dloss / ((float)a.B * (float)max(L, 1));

  int lab[CTC_MAX_PER_THREAD];
  bool skip[CTC_MAX_PER_THREAD];
#pragma unroll
  for (int k = 0; k < CTC_MAX_PER_THREAD; ++k) {
    const int s = threadIdx.x + k * NT;
    lab[k] = s < S ? sl[s] : a.blank;
    skip[k] = s < S && (s & 1) && s + 2 < S && sl[s] != sl[s + 2];
  }
  // line[s] for s in [0, S), then two -inf pads read as s + 1 / s + 2 past the end
  for (int s = threadIdx.x; s < a.Sp + 2; s += NT) { line0[s] = NEG_INF; line1[s] = NEG_INF; }
  for (int v = threadIdx.x; v < 2 * V; v += NT) acc[v] = 0.f;
  __syncthreads();
  const double* alpha = a.alpha + (int64_t)b * a.T * a.Sp;
  // alpha of the next two steps, loaded two steps ahead of their use (a step is shorter than a load)
  double nxt[CTC_MAX_PER_THREAD], nxt2[CTC_MAX_PER_THREAD];
#pragma unroll
  for (int k = 0; k < CTC_MAX_PER_THREAD; ++k) {
    const int s = threadIdx.x + k * NT;
    nxt[k] = s < S ? alpha[(int64_t)(len - 1) * a.Sp + s] : NEG_INF;
    nxt2[k] = s < S && len >= 2 ? alpha[(int64_t)(len - 2) * a.Sp + s] : NEG_INF;
  }
  double* next = line0;                      // beta_{t+1}
  double* cur = line1;                       // beta_t
  float dsum[CTC_MAX_PER_THREAD] = {0.f};                   // this thread's share of dbias (V <= CTC_MAX_STATES)
  for (int t = len - 1; t >= 0; --t) {
    const float* row = lp + (int64_t)t * V;
    float* sum = acc + (t & 1) * V;
    double al[CTC_MAX_PER_THREAD];
#pragma unroll
    for (int k = 0; k < CTC_MAX_PER_THREAD; ++k) {
      const int s = threadIdx.x + k * NT;
      al[k] = nxt[k];
      nxt[k] = nxt2[k];
      if (t > 1 && s < S) nxt2[k] = alpha[(int64_t)(t - 2) * a.Sp + s];
    }
#pragma unroll
    for (int k = 0; k < CTC_MAX_PER_THREAD; ++k) {
      const int s = threadIdx.x + k * NT;
      if (s < S) {
        const double e = (double)row[lab[k]];
        double bt;
        if (t == len - 1) bt = s >= S - 2 ? e : NEG_INF;
        else bt = lse3(next[s], next[s + 1], skip[k] ? next[s + 2] : NEG_INF) + e;
        cur[s] = bt;
        const double w = al[k] + bt + nll - e;         // log of this state's share of the class posterior (<= 0)
        if (w > NEG_INF) atomicAdd(&sum[lab[k]], fast_exp((float)w));
      }
    }
    __syncthreads();
    // classes: write the gradient of step t, clear the row for step t - 2 (the next barrier orders it)
#pragma unroll
    for (int j = 0; j < CTC_MAX_PER_THREAD; ++j) {
      const int v = threadIdx.x + j * NT;
      if (v < V) {
        const float g = (expf(row[v]) - sum[v]) * scale;
        dl[(int64_t)t * V + v] = g;
        dsum[j] += g;
        sum[v] = 0.f;
      }
    }
    double* tmp = next; next = cur; cur = tmp;
  }
  if (a.dbias) {
#pragma unroll
    for (int j = 0; j < CTC_MAX_PER_THREAD; ++j) {
      const int v = threadIdx.x + j * NT;
      if (v < V) atomicAdd(&a.dbias[v], dsum[j]);
    }
  }
}

int ctc_threads(int Sp, int V) {
  const int need = Sp > V ? Sp : V;
  return need <= 256 ? 256 : need <= 512 ? 512 : 1024;
}

bool table_in_lds(int64_t T, int64_t V) { return T * V * 4 <= CTC_LDS_TABLE_BYTES; }

int check_shape(int64_t B, int64_t T, int64_t V, int64_t Lmax) {
  if (B < 1 || T < 1 || V < 2 || Lmax < 0) return SSASR_EARG;
  if (2 * Lmax + 1 > CTC_MAX_STATES || V > CTC_MAX_STATES || B > 65535) return SSASR_EARG;
  return SSASR_OK;
}

// ---- forced alignment: the max-product lattice with back-pointers and a traceback (include/ssasr.h) ----------
// BUILD-DEFINED like the rest of this file.  The lattice runs on the RAW logits: every path visits every frame
// once, so the per-frame normaliser cannot change which path wins, and each lattice value is then one double add
// and comparisons in frame order -- a float64 restatement that does the same operations gets the same bits, which
// is why the tests demand the exact path.  The normalisers lse_t (ctc_table's formula) only enter score and
// char_logp.
//
// One workgroup per utterance, one state per thread, two LDS lines, one barrier per frame, the frame's logit
// loaded one step ahead (no table: a state reads ONE class per frame).  A step's back-pointer is two bits per
// state; a wave packs its 64 states with two ballots into two 64-bit words, so a frame's row is
// ceil(Sp / 64) * 16 bytes.  The rows stay in LDS while T * ceil(Sp / 64) * 16 <= 128 KB (T <= 819 at Sp = 601,
// T <= 512 at Sp = 1023) and go to the workspace otherwise.  The traceback is wave 0's: per 64 frames every lane
// loads its frame's words for the (at most three) 64-state groups the path can reach in 64 steps, then the 64
// dependent steps run on registers and cross-lane reads, so the chain pays one memory latency per 64 frames.
constexpr int64_t ALIGN_LDS_BP_BYTES = 128 * 1024;
constexpr int ALIGN_RED_DOUBLES = 16;                       // one partial sum per wave

struct AlignArgs {
  const float* logits;       // [B][T][V]
  const int32_t* frame_lens; // [B]
  const int32_t* y;
  int64_t y_ld;
  const int32_t* label_lens; // [B]
  int T, V, Sp, Lmax, blank;
  int groups;                // ceil(Sp / 64): 64-state groups of a back-pointer row
  double* lse;               // [B][T] the frames' log-sum-exp
  unsigned long long* bp;    // [B][T][groups][2] or nullptr when the rows fit LDS
  int32_t* path;             // [B][T]
  int32_t* first;            // [B][Lmax]
  int32_t* last;             // [B][Lmax]
  float* char_logp;          // [B][Lmax]
  double* score;             // [B]
  long long* stamps;         // [B][4] wall_clock64 at the start, before and after the traceback, at the end (tools/align_time.py)
};

template <int NT>
__device__ void align_none(const AlignArgs& a, int b) {
  for (int t = threadIdx.x; t < a.T; t += NT) a.path[(int64_t)b * a.T + t] = -1;
  for (int j = threadIdx.x; j < a.Lmax; j += NT) {
    a.first[(int64_t)b * a.Lmax + j] = -1;
    a.last[(int64_t)b * a.Lmax + j] = -1;
    a.char_logp[(int64_t)b * a.Lmax + j] = 0.f;
  }
  if (threadIdx.x == 0) a.score[b] = NEG_INF;
}

template <bool LDS_BP, int NT>
__global__ __launch_bounds__(NT) void ctc_align_kernel(AlignArgs a) {
  extern __shared__ double smem_d[];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int len = min(a.frame_lens[b], a.T), L = a.label_lens[b], S = 2 * L + 1, V = a.V;
  if (len < 1 || L < 0 || S > a.Sp) {        // nothing to align
    align_none<NT>(a, b);
    return;
  }
  double* line0 = smem_d;                    // [2 pads][Sp]
  double* line1 = line0 + ctc_line_doubles(a.Sp);
  double* red = line1 + ctc_line_doubles(a.Sp);
  unsigned long long* bp_lds = reinterpret_cast<unsigned long long*>(red + ALIGN_RED_DOUBLES);
  unsigned long long* bp = LDS_BP ? bp_lds : a.bp + (int64_t)b * a.T * a.groups * 2;
  int* sl = reinterpret_cast<int*>(bp_lds + (LDS_BP ? (int64_t)a.T * a.groups * 2 : 0));
  const float* logits = a.logits + (int64_t)b * a.T * V;
  const int32_t* yr = a.y + (int64_t)b * a.y_ld;
  double* lse = a.lse + (int64_t)b * a.T;
  int32_t* path = a.path + (int64_t)b * a.T;
  long long* stamps = a.stamps + (int64_t)b * 4;
  if (tid == 0) stamps[0] = wall_clock64();

  for (int s = tid; s < S; s += NT) sl[s] = (s & 1) ? yr[s >> 1] : a.blank;
  // the frames' normalisers, one wave per frame (ctc_table's arithmetic)
  for (int t = wave; t < len; t += NT / 64) {
    const float* row = logits + (int64_t)t * V;
    float m = -INFINITY;
    for (int v = lane; v < V; v += 64) m = fmaxf(m, row[v]);
    m = wave_max(m);
    float sum = 0.f;
    for (int v = lane; v < V; v += 64) sum += expf(row[v] - m);
    sum = wave_sum(sum);
    if (lane == 0) lse[t] = (double)m + (double)logf(sum);
  }
  __syncthreads();

  const int s = tid;
  const int lab = s < S ? sl[s] : a.blank;
  const bool skip = s < S && (s & 1) && s >= 3 && sl[s] != sl[s - 2];
  const float* col = logits + lab;
  if (tid < 2) { line0[tid] = NEG_INF; line1[tid] = NEG_INF; }
  if (s < S) line0[2 + s] = s < 2 ? (double)col[0] : NEG_INF;
  float x_next = len > 1 ? col[V] : 0.f;
  __syncthreads();
  double* prev = line0;
  double* cur = line1;
  for (int t = 1; t < len; ++t) {
    const float x = x_next;
    if (t + 1 < len) x_next = col[(int64_t)(t + 1) * V];
    int from = 0;
    if (s < S) {
      double best = prev[2 + s];                              // stay wins a tie, then s - 1, then s - 2
      const double one = prev[1 + s], two = skip ? prev[s] : NEG_INF;
      if (one > best) { best = one; from = 1; }
      if (two > best) { best = two; from = 2; }
      cur[2 + s] = best + (double)x;
    }
    const unsigned long long lo = __ballot(from & 1), hi = __ballot(from >> 1);
    if (lane == 0 && wave < a.groups) {
      unsigned long long* w = bp + ((int64_t)t * a.groups + wave) * 2;
      w[0] = lo;
      w[1] = hi;
    }
    __syncthreads();
    double* tmp = prev; prev = cur; cur = tmp;
  }
  const double end1 = prev[2 + S - 1], end2 = S > 1 ? prev[2 + S - 2] : NEG_INF;
  const double d_end = end2 > end1 ? end2 : end1;            // S - 1 wins a tie
  if (!(d_end > NEG_INF)) {                                  // the frames cannot hold the labels
    align_none<NT>(a, b);
    return;
  }
  if (tid == 0) stamps[1] = wall_clock64();
  if (wave == 0) {
    int st = end2 > end1 ? S - 2 : S - 1;
    for (int t0 = len - 1; t0 >= 0; t0 -= 64) {
      const int t = t0 - lane, top = st >> 6;
      unsigned long long m0[3] = {0, 0, 0}, m1[3] = {0, 0, 0};   // frame t's words of groups top, top - 1, top - 2
      if (t >= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (top - k >= 0) {
            const unsigned long long* w = bp + ((int64_t)t * a.groups + (top - k)) * 2;
            m0[k] = w[0];
            m1[k] = w[1];
          }
      }
      int mine = -1;
      const int n = min(64, t0 + 1);
      for (int i = 0; i < n; ++i) {                          // st falls by at most 2 per step: it stays in the three groups
        if (lane == i) mine = st;
        const int k = top - (st >> 6);
        const unsigned long long lo = __shfl(k == 0 ? m0[0] : k == 1 ? m0[1] : m0[2], i);
        const unsigned long long hi = __shfl(k == 0 ? m1[0] : k == 1 ? m1[1] : m1[2], i);
        const int sh = st & 63;
        st = max(st - (int)((lo >> sh) & 1) - 2 * (int)((hi >> sh) & 1), 0);
      }
      if (t >= 0) path[t] = mine;
    }
    if (tid == 0) stamps[2] = wall_clock64();
  }
  __syncthreads();
  // derived outputs, in parallel from the path
  for (int t = len + tid; t < a.T; t += NT) path[t] = -1;
  int32_t* first = a.first + (int64_t)b * a.Lmax;
  int32_t* last = a.last + (int64_t)b * a.Lmax;
  float* clp = a.char_logp + (int64_t)b * a.Lmax;
  for (int j = L + tid; j < a.Lmax; j += NT) { first[j] = -1; last[j] = -1; clp[j] = 0.f; }
  double part = 0.0;
  for (int t = tid; t < len; t += NT) {
    part += lse[t];
    const int q = path[t];
    if (q & 1) {
      if (t == 0 || path[t - 1] != q) first[q >> 1] = t;
      if (t == len - 1 || path[t + 1] != q) last[q >> 1] = t;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off);
  if (lane == 0) red[wave] = part;
  __syncthreads();
  if (tid == 0) {
    double total = 0.0;
    for (int w = 0; w < NT / 64; ++w) total += red[w];
    a.score[b] = d_end - total;
  }
  for (int j = tid; j < L; j += NT) {
    const float* cj = logits + yr[j];
    double acc = 0.0;
    const int t_end = min(last[j], len - 1);
    for (int t = max(first[j], 0); t <= t_end; ++t) acc += (double)cj[(int64_t)t * V] - lse[t];
    clp[j] = (float)acc;
  }
  if (tid == 0) stamps[3] = wall_clock64();
}

int align_groups(int64_t Lmax) { return (int)((2 * Lmax + 1 + 63) / 64); }

bool align_bp_in_lds(int64_t T, int64_t Lmax) { return T * align_groups(Lmax) * 16 <= ALIGN_LDS_BP_BYTES; }

int align_check_shape(int64_t B, int64_t T, int64_t V, int64_t Lmax) {
  if (check_shape(B, T, V, Lmax) != SSASR_OK || T > INT32_MAX) return SSASR_EARG;
  return SSASR_OK;
}

// ---- CTC-only decoding: best path and prefix beam search (include/ssasr.h) -----------------------------------------
// BUILD-DEFINED like the rest of this file.  One workgroup of 256 threads per utterance, a serial loop over its
// frames.  The prefix search's frame body, its limits and its argument block live in ctc_prefix.h, shared with the
// graph kernel below and with infer.hip's CharLM kernel; this file holds the best path and the two kernels' set-up.
constexpr int DEC_NT = 256;
constexpr int DEC_WAVES = DEC_NT / 64;
constexpr int DEC_MAX_V_BEST = 1024;

// K = 0 (the best path): text is [B][T] the frames' labels, the outputs hold one hypothesis a row
using DecodeArgs = ctc_prefix::Args;

__global__ __launch_bounds__(DEC_NT) void ctc_best_path_kernel(DecodeArgs a) {
  __shared__ double red[DEC_WAVES];
  __shared__ int cnt[DEC_NT];
  __shared__ int n_sh;
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int len = max(min(a.frame_lens[b], a.T), 0), V = a.V;
  const float* logits = a.logits + (int64_t)b * a.T * V;
  int32_t* lab = a.text + (int64_t)b * a.T;
  int32_t* out = a.chars + (int64_t)b * a.T;
  double part = 0.0;
  for (int t = wave; t < len; t += DEC_WAVES) {
    const float* row = logits + (int64_t)t * V;
    float m = lane < V ? row[lane] : -INFINITY;
    int am = lane < V ? lane : INT32_MAX;
    for (int v = lane + 64; v < V; v += 64) {
      const float x = row[v];
      if (x > m) { m = x; am = v; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {                // the largest value, the lowest index among equals
      const float om = __shfl_xor(m, off);
      const int oa = __shfl_xor(am, off);
      if (om > m || (om == m && oa < am)) { m = om; am = oa; }
    }
    float s = 0.f;
    for (int v = lane; v < V; v += 64) s += expf(row[v] - m);
    s = wave_sum(s);
    part += (double)row[am] - ((double)m + (double)logf(s));
    if (lane == 0) lab[t] = am;
  }
  if (lane == 0) red[wave] = part;
  __syncthreads();
  // merge repeats, drop blanks: a thread counts the kept labels of its run of frames, then writes them behind
  // those of the threads before it
  const int chunk = (len + DEC_NT - 1) / DEC_NT;
  const int t0 = min(tid * chunk, len), t1 = min(t0 + chunk, len);
  int keep = 0;
  for (int t = t0; t < t1; ++t) keep += lab[t] != a.blank && (t == 0 || lab[t] != lab[t - 1]);
  cnt[tid] = keep;
  __syncthreads();
  int at = 0;
  for (int i = 0; i < tid; ++i) at += cnt[i];
  if (tid == DEC_NT - 1) n_sh = at + keep;
  for (int t = t0; t < t1; ++t)
    if (lab[t] != a.blank && (t == 0 || lab[t] != lab[t - 1])) out[at++] = lab[t];
  __syncthreads();
  const int n = n_sh;
  for (int i = n + tid; i < a.T; i += DEC_NT) out[i] = 0;
  if (tid == 0) {
    double total = 0.0;
    for (int w = 0; w < DEC_WAVES; ++w) total += red[w];
    a.n_chars[b] = n;
    a.scores[b] = (float)total;
    a.n_hyps[b] = 1;
  }
}

// the prefix search with no term beside the CTC total: ctc_prefix.h's body as it is
__global__ __launch_bounds__(DEC_NT) void ctc_prefix_beam_kernel(DecodeArgs a) {
  __shared__ ctc_prefix::State<DEC_NT, ctc_prefix::NoTerm> s;
  ctc_prefix::NoTerm term;
  ctc_prefix::search(a, term, s);
}

// K = 0: the best path's limits; K >= 1: the prefix search's
int decode_check_shape(int64_t B, int64_t T, int64_t V, int64_t K) {
  if (K != 0) return ctc_prefix::shape_ok(B, T, V, K) ? SSASR_OK : SSASR_EARG;
  if (B < 1 || B > ctc_prefix::kMaxB || T < 1 || T > ctc_prefix::kMaxT || V < 2 || V > DEC_MAX_V_BEST) return SSASR_EARG;
  return SSASR_OK;
}


// ---- the prefix beam search with a character graph in the ranking (include/ssasr.h, ssasr_ctc_decode_graph) --------
// ctc_prefix.h's frame body with GraphTerm: beside g_b / g_n every member carries the graph's state after its text
// (int32) and, in the body's acc, G, the sum of the arcs taken (double).  The rows next[state][.] and arc[state][.] of
// a member sit in LDS, [slot][64], from the frame after the member entered a beam until it leaves: a kept member keeps
// its slot, so the candidate loop and the winners' update read LDS alone.  The only global reads of the tables are the
// rows of a frame's new members: issued in after_commit, once the winners are known, a wave per member, and stored to
// LDS as they arrive; the next frame's two barriers lie before their first reader.  (Holding them in registers over
// the frame boundary and storing after the next frame's parent look-up measured no faster: DESIGN.md 4.22.)  Every
// state read from the table is clamped to [0, S - 1]: a malformed table gives wrong scores, no stray read.

struct GraphArgs {
  DecodeArgs d;
  const int32_t* next;       // [S][V]
  const float* arc;          // [S][V]
  const float* fin;          // [S]
  int S, start;
  float graph_weight, length_bonus;
  float *ctc_scores, *graph_scores;   // [B][K]
};

struct GraphTerm : ctc_prefix::Scored {
  struct Mem : ctc_prefix::ScoredMem {
    int gst[2][ctc_prefix::kMaxK];                           // the graph's state after the text
    float arow[ctc_prefix::kMaxK][64];                       // [slot]: arc[state][.]
    int nrow[ctc_prefix::kMaxK][64];                         // [slot]: next[state][.]
  };
  const GraphArgs& g;
  int s_max;

  __device__ explicit GraphTerm(const GraphArgs& ga)
      : Scored{ga.graph_weight != 0.f, ga.length_bonus != 0.f, (double)ga.graph_weight, (double)ga.length_bonus,
               ga.ctc_scores, ga.graph_scores},
        g(ga), s_max(ga.S - 1) {}

  __device__ void load_rows(Mem& m, int slot, int state, int V) const {   // one wave
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)state * V;
    m.arow[slot][lane] = lane < V ? g.arc[row + lane] : 0.f;
    m.nrow[slot][lane] = lane < V ? g.next[row + lane] : 0;
  }
  __device__ void init(Mem& m, int V) const {                // the empty text's rows: the start state's
    if (threadIdx.x == 0) m.gst[0][0] = on ? g.start : 0;
    if (on && threadIdx.x < 64) load_rows(m, 0, g.start, V);
  }
  __device__ double step(const Mem& m, int cur, int u, int c) const { return (double)m.arow[m.slot[cur][u]][c]; }
  __device__ void keep(Mem& m, int cur, int nxt, int j, int w) const { m.gst[nxt][j] = m.gst[cur][w]; }
  __device__ void inherit(Mem& m, int cur, int nxt, int j, int u, int c) const {
    m.gst[nxt][j] = on ? min(max(m.nrow[m.slot[cur][u]][c], 0), s_max) : 0;
  }
  // the new members' rows: a wave per member; two barriers of the next frame lie before their first reader
  template <class S>
  __device__ void after_commit(S& s, int, int nxt, int, int V) const {
    Mem& m = s.tm;
    const int ne = on ? m.n_ext : 0;
    for (int e = threadIdx.x >> 6; e < ne; e += DEC_WAVES) {
      const int j = m.ext[e];
      load_rows(m, m.slot[nxt][j], m.gst[nxt][j], V);
    }
  }
  __device__ bool has_end() const { return true; }
  __device__ double end(const Mem& m, int cur, int j) const { return (double)g.fin[min(max(m.gst[cur][j], 0), s_max)]; }
};

__global__ __launch_bounds__(DEC_NT) void ctc_prefix_beam_graph_kernel(GraphArgs g) {
  __shared__ ctc_prefix::State<DEC_NT, GraphTerm> s;
  GraphTerm term(g);
  ctc_prefix::search(g.d, term, s);
}

constexpr int GRAPH_MAX_STATES = 1 << 20;

// ---- the prefix beam search over a lexicon with a word n-gram LM (include/ssasr.h, ssasr_ctc_decode_word) ----------
// ctc_prefix.h's frame body with WordTerm.  A member's state is the pair (trie node, word-LM state), two int32 in LDS;
// its two rows sit in LDS [slot][64] exactly as GraphTerm's do, filled in after_commit by one wave per new member from
// child[node][.] / carc[node][.].  The one entry that is no dense read is the space class's: where a word ends at the
// node the wave looks word[node] up in the LM state's row, backing off until it is found (state 0's row is dense, so
// that ends), and stores the arc (float)(pen[node] + lp) in the row and the LM state behind it beside the row (hsp),
// so the candidate loop and the winners' update read LDS alone.  The look-up in a row is a 64-way search: every lane
// probes one cut of the row, the ballot picks the segment, and a row of 200k words is down to <= 64 entries after two
// rounds; the last round compares them all at once.  The end term does the same look-up once per member, one thread
// each with a binary search, since no barrier lies between the last frame's hook and the ranking.  Every node, state
// and row bound read from a table is clamped into range: a malformed table gives wrong scores, no stray read.
constexpr int WORD_MAX_NODES = 1 << 20;
constexpr int WORD_SEARCH_ROUNDS = 32;

struct WordArgs {
  DecodeArgs d;
  const int32_t* child;      // [N][V]
  const float* carc;         // [N][V]
  const int32_t* word;       // [N]
  const float* pen;          // [N]
  const int32_t* off;        // [H + 1]
  const int32_t* wid;        // [E]
  const float* wlp;          // [E]
  const int32_t* wnext;      // [E]
  const float* bow;          // [H]
  const int32_t* bnext;      // [H]
  const float* eos;          // [H]
  int N, H, W, E, sp;
  float graph_weight, length_bonus;
  float *ctc_scores, *graph_scores;   // [B][K]
};

struct WordHit {
  double lp;                 // the backed-off log-probability, -inf: a malformed table
  int next;                  // the LM state after the word
};

struct WordTerm : ctc_prefix::Scored {
  struct Mem : ctc_prefix::ScoredMem {
    int node[2][ctc_prefix::kMaxK];                          // the trie node after the text
    int hst[2][ctc_prefix::kMaxK];                           // the word LM's state after the text's last space
    float arow[ctc_prefix::kMaxK][64];                       // [slot]: carc[node][.], the space entry looked up
    int nrow[ctc_prefix::kMaxK][64];                         // [slot]: child[node][.], the space entry the root
    int hsp[ctc_prefix::kMaxK];                              // [slot]: the LM state behind the space arc
  };
  const WordArgs& g;

  __device__ explicit WordTerm(const WordArgs& wa)
      : Scored{wa.graph_weight != 0.f, wa.length_bonus != 0.f, (double)wa.graph_weight, (double)wa.length_bonus,
               wa.ctc_scores, wa.graph_scores},
        g(wa) {}

  // the entry of word w in [lo, hi), -1: none.  The whole wave calls it with the same arguments.
  __device__ int find_wave(int lo, int hi, int w) const {
    const int lane = threadIdx.x & 63;
    for (int r = 0; r < WORD_SEARCH_ROUNDS && hi - lo > 64; ++r) {
      const int step = (hi - lo + 63) >> 6;                  // 64 cuts; the segment after the last one <= w has w
      const int64_t i = lo + (int64_t)lane * step;
      const int cnt = __popcll(__ballot(i < hi && g.wid[i < hi ? i : lo] <= w));
      if (cnt == 0) return -1;
      lo += (cnt - 1) * step;                                // cnt lanes had i < hi: lo stays below hi
      hi = min(lo + step, hi);
    }
    const int i = lo + lane;
    const unsigned long long hit = __ballot(i < hi && g.wid[i < hi ? i : lo] == w);
    return hit ? lo + __ffsll((long long)hit) - 1 : -1;
  }
  // the same by one thread
  __device__ int find_thread(int lo, int hi, int w) const {
    for (int r = 0; r < WORD_SEARCH_ROUNDS && lo < hi; ++r) {
      const int mid = lo + ((hi - lo) >> 1);
      const int v = g.wid[mid];
      if (v == w) return mid;
      if (v < w) lo = mid + 1; else hi = mid;
    }
    return -1;
  }
  // lookup(h, w) of the header: WAVE: by the whole wave, else by the calling thread; the same sums in the same order
  template <bool WAVE>
  __device__ WordHit lookup(int h, int w) const {
    double acc = 0.0;
    w = min(w, g.W - 1);
    for (int r = 0; r < SSASR_WORD_MAX_ORDER; ++r) {
      const int lo = min(max(g.off[h], 0), g.E), hi = min(max(g.off[h + 1], lo), g.E);
      int e;
      if (h == 0) e = min(lo + w, g.E - 1);                  // the dense row
      else if (lo >= hi) e = -1;
      else e = WAVE ? find_wave(lo, hi, w) : find_thread(lo, hi, w);
      if (e >= 0) return WordHit{acc + (double)g.wlp[e], min(max(g.wnext[e], 0), g.H - 1)};
      acc += (double)g.bow[h];
      const int b = g.bnext[h];
      if (b < 0) break;
      h = min(b, g.H - 1);
    }
    return WordHit{ctc_prefix::kNegInf, 0};
  }
  // the space arc out of (node, h), a word ending at the node
  template <bool WAVE>
  __device__ float space_arc(int node, int h, int w, int& h_next) const {
    const WordHit hit = lookup<WAVE>(h, w);
    h_next = hit.next;
    return (float)((double)g.pen[node] + hit.lp);
  }

  __device__ void load_rows(Mem& m, int slot, int node, int h, int V) const {   // one wave
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)node * V;
    const bool dense = lane < V && lane != g.sp && lane != g.d.blank;
    float a = dense ? g.carc[row + lane] : 0.f;
    const int nx = dense ? g.child[row + lane] : 0;
    const int w = g.word[node];
    int h_next = 0;
    if (w >= 0) {                                            // the same for the whole wave
      const float sa = space_arc<true>(node, h, w, h_next);
      if (lane == g.sp) a = sa;
    } else if (lane == g.sp) {
      a = -INFINITY;
    }
    m.arow[slot][lane] = a;
    m.nrow[slot][lane] = nx;
    if (lane == 0) m.hsp[slot] = h_next;
  }
  __device__ void init(Mem& m, int V) const {                // the empty text: the root, the empty history
    if (threadIdx.x == 0) { m.node[0][0] = 0; m.hst[0][0] = 0; }
    if (on && threadIdx.x < 64) load_rows(m, 0, 0, 0, V);
  }
  __device__ double step(const Mem& m, int cur, int u, int c) const { return (double)m.arow[m.slot[cur][u]][c]; }
  __device__ void keep(Mem& m, int cur, int nxt, int j, int w) const {
    m.node[nxt][j] = m.node[cur][w];
    m.hst[nxt][j] = m.hst[cur][w];
  }
  __device__ void inherit(Mem& m, int cur, int nxt, int j, int u, int c) const {
    const int sl = m.slot[cur][u];
    m.node[nxt][j] = on ? min(max(m.nrow[sl][c], 0), g.N - 1) : 0;
    m.hst[nxt][j] = on ? (c == g.sp ? m.hsp[sl] : m.hst[cur][u]) : 0;
  }
  // the new members' rows: a wave per member; two barriers of the next frame lie before their first reader
  template <class S>
  __device__ void after_commit(S& s, int, int nxt, int, int V) const {
    Mem& m = s.tm;
    const int ne = on ? m.n_ext : 0;
    for (int e = threadIdx.x >> 6; e < ne; e += DEC_WAVES) {
      const int j = m.ext[e];
      load_rows(m, m.slot[nxt][j], m.node[nxt][j], m.hst[nxt][j], V);
    }
  }
  __device__ bool has_end() const { return true; }
  // fin(node, h): the rows of the last frame's new members may still be in flight, so the member looks up again
  __device__ double end(const Mem& m, int cur, int j) const {
    const int node = m.node[cur][j], h = m.hst[cur][j];
    const int w = g.word[node];
    if (w < 0) return (double)g.pen[node] + (double)g.eos[h];
    int h_next;
    const float sa = space_arc<false>(node, h, w, h_next);
    return (double)sa + (double)g.eos[h_next];
  }
};

__global__ __launch_bounds__(DEC_NT) void ctc_prefix_beam_word_kernel(WordArgs g) {
  __shared__ ctc_prefix::State<DEC_NT, WordTerm> s;
  WordTerm term(g);
  ctc_prefix::search(g.d, term, s);
}

}  // namespace

extern "C" int64_t ssasr_ctc_decode_ws_bytes(int64_t B, int64_t T, int64_t V, int64_t K) {
  if (decode_check_shape(B, T, V, K) != SSASR_OK) return 0;
  return (K == 0 ? B * T : B * 2 * K * T) * 4;
}

extern "C" int ssasr_ctc_decode(const float* logits, const int32_t* frame_lens, int64_t B, int64_t T, int64_t V,
                                int64_t K, int blank, void* ws, int64_t ws_bytes, int32_t* chars, int32_t* n_chars,
                                float* scores, int32_t* n_hyps, void* stream) {
  if (!logits || !frame_lens || !ws || !chars || !n_chars || !scores || !n_hyps) return SSASR_EARG;
  if (decode_check_shape(B, T, V, K) != SSASR_OK || blank < 0 || blank >= V) return SSASR_EARG;
  if ((reinterpret_cast<uintptr_t>(ws) & 7) || ws_bytes < ssasr_ctc_decode_ws_bytes(B, T, V, K)) return SSASR_EARG;
  const DecodeArgs a = ctc_prefix::make_args(logits, frame_lens, T, V, K, blank, ws, chars, n_chars, scores, n_hyps);
  void (*fn)(DecodeArgs) = K == 0 ? ctc_best_path_kernel : ctc_prefix_beam_kernel;
  hipLaunchKernelGGL(fn, dim3((unsigned)B), dim3(DEC_NT), 0, (hipStream_t)stream, a);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}

extern "C" int64_t ssasr_ctc_decode_graph_ws_bytes(int64_t B, int64_t T, int64_t V, int64_t K) {
  if (!ctc_prefix::shape_ok(B, T, V, K)) return 0;
  return B * 2 * K * T * 4;
}

extern "C" int ssasr_ctc_decode_graph(const float* logits, const int32_t* frame_lens, int64_t B, int64_t T, int64_t V,
                                      int64_t K, int blank, void* ws, int64_t ws_bytes, int32_t* chars,
                                      int32_t* n_chars, float* scores, int32_t* n_hyps, const ssasr_char_graph* graph,
                                      float graph_weight, float length_bonus, float* ctc_scores, float* graph_scores,
                                      void* stream) {
  if (!logits || !frame_lens || !ws || !chars || !n_chars || !scores || !n_hyps || !ctc_scores || !graph_scores)
    return SSASR_EARG;
  if (!std::isfinite(graph_weight) || graph_weight < 0.f || !std::isfinite(length_bonus)) return SSASR_EARG;
  if (!ctc_prefix::shape_ok(B, T, V, K) || blank < 0 || blank >= V) return SSASR_EARG;
  if (graph_weight != 0.f && !graph) return SSASR_EARG;
  if (graph && (!graph->next || !graph->arc || !graph->fin || graph->V != V || graph->S < 1 ||
                graph->S > GRAPH_MAX_STATES || graph->start < 0 || graph->start >= graph->S))
    return SSASR_EARG;
  if ((reinterpret_cast<uintptr_t>(ws) & 7) || ws_bytes < ssasr_ctc_decode_graph_ws_bytes(B, T, V, K)) return SSASR_EARG;
  GraphArgs g{};
  g.d = ctc_prefix::make_args(logits, frame_lens, T, V, K, blank, ws, chars, n_chars, scores, n_hyps);
  g.graph_weight = graph_weight; g.length_bonus = length_bonus;
  g.ctc_scores = ctc_scores; g.graph_scores = graph_scores;
  g.S = 1;
  if (graph && graph_weight != 0.f) {                        // weight 0: the tables are unread
    g.next = graph->next; g.arc = graph->arc; g.fin = graph->fin;
    g.S = graph->S; g.start = graph->start;
  }
  hipLaunchKernelGGL(ctc_prefix_beam_graph_kernel, dim3((unsigned)B), dim3(DEC_NT), 0,
                     (hipStream_t)stream, g);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}

extern "C" int64_t ssasr_ctc_decode_word_ws_bytes(int64_t B, int64_t T, int64_t V, int64_t K) {
  if (!ctc_prefix::shape_ok(B, T, V, K)) return 0;
  return B * 2 * K * T * 4;
}

extern "C" int ssasr_ctc_decode_word(const float* logits, const int32_t* frame_lens, int64_t B, int64_t T, int64_t V,
                                     int64_t K, int blank, void* ws, int64_t ws_bytes, int32_t* chars,
                                     int32_t* n_chars, float* scores, int32_t* n_hyps, const ssasr_word_graph* graph,
                                     float graph_weight, float length_bonus, float* ctc_scores, float* graph_scores,
                                     void* stream) {
  if (!logits || !frame_lens || !ws || !chars || !n_chars || !scores || !n_hyps || !ctc_scores || !graph_scores)
    return SSASR_EARG;
  if (!std::isfinite(graph_weight) || graph_weight < 0.f || !std::isfinite(length_bonus)) return SSASR_EARG;
  if (!ctc_prefix::shape_ok(B, T, V, K) || blank < 0 || blank >= V) return SSASR_EARG;
  if (graph_weight != 0.f && !graph) return SSASR_EARG;
  if (graph) {
    const ssasr_word_graph& w = *graph;
    if (!w.child || !w.carc || !w.word || !w.pen || !w.off || !w.wid || !w.wlp || !w.wnext || !w.bow || !w.bnext ||
        !w.eos)
      return SSASR_EARG;
    if (w.V != V || w.sp < 0 || w.sp >= V || w.sp == blank) return SSASR_EARG;
    if (w.N < 1 || w.N > WORD_MAX_NODES || w.H < 1 || w.H > WORD_MAX_NODES || w.W < 1 || w.W > WORD_MAX_NODES ||
        w.E < w.W)
      return SSASR_EARG;
  }
  if ((reinterpret_cast<uintptr_t>(ws) & 7) || ws_bytes < ssasr_ctc_decode_word_ws_bytes(B, T, V, K)) return SSASR_EARG;
  WordArgs g{};
  g.d = ctc_prefix::make_args(logits, frame_lens, T, V, K, blank, ws, chars, n_chars, scores, n_hyps);
  g.graph_weight = graph_weight; g.length_bonus = length_bonus;
  g.ctc_scores = ctc_scores; g.graph_scores = graph_scores;
  g.N = g.H = g.W = g.E = 1;
  if (graph && graph_weight != 0.f) {                        // weight 0: the tables are unread
    g.child = graph->child; g.carc = graph->carc; g.word = graph->word; g.pen = graph->pen;
    g.off = graph->off; g.wid = graph->wid; g.wlp = graph->wlp; g.wnext = graph->wnext;
    g.bow = graph->bow; g.bnext = graph->bnext; g.eos = graph->eos;
    g.N = graph->N; g.H = graph->H; g.W = graph->W; g.E = graph->E; g.sp = graph->sp;
  }
  hipLaunchKernelGGL(ctc_prefix_beam_word_kernel, dim3((unsigned)B), dim3(DEC_NT), 0, (hipStream_t)stream, g);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}

extern "C" int64_t ssasr_ctc_align_ws_bytes(int64_t B, int64_t T, int64_t V, int64_t Lmax) {
  if (align_check_shape(B, T, V, Lmax) != SSASR_OK) return 0;
  return B * T * 8 + (align_bp_in_lds(T, Lmax) ? 0 : B * T * align_groups(Lmax) * 16) + B * 32;   // lse, back-pointers, stamps
}

extern "C" int ssasr_ctc_align(const float* logits, const int32_t* frame_lens, const int32_t* y, int64_t y_ld,
                               const int32_t* label_lens, int64_t B, int64_t T, int64_t V, int64_t Lmax, int blank,
                               void* ws, int64_t ws_bytes, int32_t* path, int32_t* first, int32_t* last,
                               float* char_logp, double* score, void* stream) {
  if (!logits || !frame_lens || !y || !label_lens || !ws || !path || !score) return SSASR_EARG;
  if (align_check_shape(B, T, V, Lmax) != SSASR_OK || blank < 0 || blank >= V) return SSASR_EARG;
  if (Lmax > 0 && (!first || !last || !char_logp)) return SSASR_EARG;
  if ((reinterpret_cast<uintptr_t>(ws) & 7) || ws_bytes < ssasr_ctc_align_ws_bytes(B, T, V, Lmax)) return SSASR_EARG;
  hipStream_t st = (hipStream_t)stream;
  AlignArgs a{};
  a.logits = logits; a.frame_lens = frame_lens; a.y = y; a.y_ld = y_ld; a.label_lens = label_lens;
  a.T = (int)T; a.V = (int)V; a.Sp = (int)(2 * Lmax + 1); a.Lmax = (int)Lmax; a.blank = blank;
  a.groups = align_groups(Lmax);
  a.lse = reinterpret_cast<double*>(ws);
  const bool in_lds = align_bp_in_lds(T, Lmax);
  a.bp = in_lds ? nullptr : reinterpret_cast<unsigned long long*>(a.lse + B * T);
  a.stamps = reinterpret_cast<long long*>(a.lse + B * T + (in_lds ? 0 : B * T * a.groups * 2));
  a.path = path; a.first = first; a.last = last; a.char_logp = char_logp; a.score = score;
  const size_t lds = (size_t)(a.Sp + 2) * 16 + ALIGN_RED_DOUBLES * 8 + (in_lds ? (size_t)T * a.groups * 16 : 0) +
                     (size_t)a.Sp * 4;
  const int nt = ctc_threads(a.Sp, 0);                       // one state per thread; classes are read by whole waves
  void (*fn)(AlignArgs) = nullptr;
  if (nt == 256) fn = in_lds ? ctc_align_kernel<true, 256> : ctc_align_kernel<false, 256>;
  else if (nt == 512) fn = in_lds ? ctc_align_kernel<true, 512> : ctc_align_kernel<false, 512>;
  else fn = in_lds ? ctc_align_kernel<true, 1024> : ctc_align_kernel<false, 1024>;
  SSASR_HIP(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(fn, dim3((unsigned)B), dim3(nt), lds, st, a);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}

extern "C" int64_t ssasr_ctc_ws_floats(int64_t B, int64_t T, int64_t V, int64_t Lmax) {
  if (check_shape(B, T, V, Lmax) != SSASR_OK) return 0;
  return 2 * (B * T * (2 * Lmax + 1) + B) + (table_in_lds(T, V) ? 0 : B * T * V);   // lattice and nll are doubles
}

extern "C" int ssasr_ctc_loss_fwd(const float* logits, const int32_t* frame_lens, const int32_t* y, int64_t y_ld,
                                  const int32_t* label_lens, int64_t B, int64_t T, int64_t V, int64_t Lmax,
                                  int blank, float* ws, float* loss, void* stream) {
  if (!logits || !frame_lens || !y || !label_lens || !ws || !loss) return SSASR_EARG;
  if (reinterpret_cast<uintptr_t>(ws) & 7) return SSASR_EARG;
  if (check_shape(B, T, V, Lmax) != SSASR_OK || blank < 0 || blank >= V) return SSASR_EARG;
  hipStream_t st = (hipStream_t)stream;
  CtcArgs a{};
  a.logits = logits; a.frame_lens = frame_lens; a.y = y; a.y_ld = y_ld; a.label_lens = label_lens;
  a.T = (int)T; a.V = (int)V; a.Sp = (int)(2 * Lmax + 1); a.blank = blank; a.B = (int)B;
  a.alpha = reinterpret_cast<double*>(ws);
  a.nll = a.alpha + B * T * a.Sp;
  const bool in_lds = table_in_lds(T, V);
  a.table = in_lds ? nullptr : reinterpret_cast<float*>(a.nll + B);
  const size_t lds = (size_t)(a.Sp + 2) * 16 + (size_t)a.Sp * 4 + (in_lds ? (size_t)T * V * 4 : 0);
  const int nt = ctc_threads(a.Sp, a.V);
  void (*fn)(CtcArgs) = nullptr;
  if (nt == 256) fn = in_lds ? ctc_alpha_kernel<true, 256> : ctc_alpha_kernel<false, 256>;
  else if (nt == 512) fn = in_lds ? ctc_alpha_kernel<true, 512> : ctc_alpha_kernel<false, 512>;
  else fn = in_lds ? ctc_alpha_kernel<true, 1024> : ctc_alpha_kernel<false, 1024>;
  SSASR_HIP(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(fn, dim3((unsigned)B), dim3(nt), lds, st, a);
  SSASR_LAUNCH_CHECK();
  hipLaunchKernelGGL(ctc_mean_kernel, dim3(1), dim3(64), 0, st, a.nll, label_lens, (int)B, loss);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}

extern "C" int ssasr_ctc_loss_bwd(const float* logits, const int32_t* frame_lens, const int32_t* y, int64_t y_ld,
                                  const int32_t* label_lens, int64_t B, int64_t T, int64_t V, int64_t Lmax,
                                  int blank, float* ws, const float* dloss, float* dlogits, float* dbias,
                                  void* stream) {
  if (!logits || !frame_lens || !y || !label_lens || !ws || !dloss || !dlogits) return SSASR_EARG;
  if (reinterpret_cast<uintptr_t>(ws) & 7) return SSASR_EARG;
  if (check_shape(B, T, V, Lmax) != SSASR_OK || blank < 0 || blank >= V) return SSASR_EARG;
  hipStream_t st = (hipStream_t)stream;
  CtcArgs a{};
  a.logits = logits; a.frame_lens = frame_lens; a.y = y; a.y_ld = y_ld; a.label_lens = label_lens;
  a.T = (int)T; a.V = (int)V; a.Sp = (int)(2 * Lmax + 1); a.blank = blank; a.B = (int)B;
  a.alpha = reinterpret_cast<double*>(ws);
  a.nll = a.alpha + B * T * a.Sp;
  const bool in_lds = table_in_lds(T, V);
  a.table = in_lds ? nullptr : reinterpret_cast<float*>(a.nll + B);
  a.dloss = dloss; a.dlogits = dlogits; a.dbias = dbias;
  const size_t lds = (size_t)(a.Sp + 2) * 16 + (size_t)(a.Sp + 2 * V) * 4 + (in_lds ? (size_t)T * V * 4 : 0);
  const int nt = ctc_threads(a.Sp, a.V);
  void (*fn)(CtcArgs) = nullptr;
  if (nt == 256) fn = in_lds ? ctc_beta_kernel<true, 256> : ctc_beta_kernel<false, 256>;
  else if (nt == 512) fn = in_lds ? ctc_beta_kernel<true, 512> : ctc_beta_kernel<false, 512>;
  else fn = in_lds ? ctc_beta_kernel<true, 1024> : ctc_beta_kernel<false, 1024>;
  SSASR_HIP(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(fn, dim3((unsigned)B), dim3(nt), lds, st, a);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}
