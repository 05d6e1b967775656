// CTC segmentation of long recordings (include/ssasr.h, "CTC segmentation"): the max-product lattice of
// ssasr_ctc_align on NORMALISED values with a free start and a free end, for lattices of up to 16,383 states.
// BUILD-DEFINED like ctc.hip.  gfx950 only.
//
// One workgroup per recording, one launch, no exchange between workgroups, no spins; every loop is bounded by len,
// S, V or Nmax.  The frame loop is serial.  A thread owns a contiguous block of P states, whose values live in
// registers.  P = 1 reads its two left neighbours' values from an LDS line, as ctc_align_kernel does.  P = 8 / 16
// blocks start at an even state, so only the block's first two states look outside it, and both at the SAME state:
// the left neighbour's top one (s - 1 of the block's blank, s - 2 of its first label).  A thread therefore hands one
// value per frame to its right neighbour through the LDS line, double-buffered, one barrier per frame.  States
// alternate blank / label, so a thread reads the blank's logit once and P / 2 label logits per frame, each loaded one
// frame ahead.
//
// The free start is a virtual state -1 whose value is always 0: it sits in the LDS lines' two pad words (-inf, 0),
// where state 0 finds it as its s - 1 and state 1 as its s - 2.  Both exist for no real state (state 0 has no s - 1,
// state 1 no s - 2), so the back-pointer codes stay 0 (stay), 1 (s - 1), 2 (s - 2), the start has the LAST place of
// the tie rule by construction, and the traceback has reached the start when it steps below state 0.
//
// Back-pointers: two bits per state and frame, 16 bytes per 64 states, always in the workspace.  P = 1: a wave's two
// ballots, {low bits, high bits}.  P = 8 / 16: each thread stores one 16- / 32-bit word {P low bits, P high bits}, so
// a wave's store is contiguous.  The traceback is ctc_align_kernel's: wave 0, 64 frames per chunk, every lane loads
// its frame's words for the three 64-state groups that the path can reach, then 64 steps on registers.
//
// SKIP (ssasr_ctc_segment_skip): the same kernel with utterance skips and a filler.  The junction J_n is the blank
// state 2 * utt_ends[n - 1] (J_0 = 0).  A thread finds the junctions among its blanks before the frame loop: a mask
// and the index of the first (the others follow it, so no register is indexed at run time).  The owner of J_n stores
// its new value to jv[frame parity][n] in LDS, the owner of J_{n+1} reads the other buffer in the next frame and
// offers it, plus skip_penalty, where a label state offers s - 2: the frame's one barrier orders both, as it orders
// the lines.  A junction's emission is max(blank, f_t + fill_penalty), f_t formed with lse_t.  Code 2 at a junction
// is the skip; the traceback then jumps to J_n, which leaves the three prefetched groups, and restarts its chunk there.
#include <math.h>

#include <type_traits>

#include "../../include/ssasr.h"
#include "common.h"

namespace {

constexpr double NEG_INF = -INFINITY;
constexpr int SEG_MAX_STATES = 16384;
constexpr int SEG_MAX_T = 32768;
constexpr int SEG_MAX_V = 1024;

struct SegArgs {
  const float* logits;       // [B][T][V]
  const int32_t* frame_lens; // [B]
  const int32_t* y;
  int64_t y_ld;
  const int32_t* label_lens; // [B]
  const int32_t* utt_ends;   // [B][utt_ld]
  int64_t utt_ld;
  const int32_t* n_utts;     // [B]
  int T, V, Sp, Lmax, Nmax, window, blank;
  int groups;                // ceil(Sp / 64): 64-state groups of a back-pointer row
  double* lse;               // [B][T] the frames' log-sum-exp
  double* q;                 // [B][T] lp[t][lab(path[t])] of the scored frames
  unsigned long long* bp;    // [B][T][groups][2]
  int32_t* path;             // [B][T]
  int32_t* first;            // [B][Lmax]
  int32_t* last;             // [B][Lmax]
  float* char_logp;          // [B][Lmax]
  double* score;             // [B]
  int32_t* utt_first;        // [B][Nmax]
  int32_t* utt_last;         // [B][Nmax]
  float* utt_conf;           // [B][Nmax]
  double* fws;               // [B][T] SKIP: f_t, the log-probability that the frame is some speech
  int32_t* utt_skipped;      // [B][Nmax] SKIP
  int32_t* is_fill;          // [B][T] SKIP
  double skip_pen, fill_pen; // SKIP: <= 0 or -inf
  long long* stamps;         // [B][4] wall_clock64 at the start, before and after the traceback, at the end (tools/segment_time.py)
};

template <int NT, bool SKIP>
__device__ void seg_none(const SegArgs& a, int b) {
  for (int t = threadIdx.x; t < a.T; t += NT) {
    a.path[(int64_t)b * a.T + t] = -1;
    if (SKIP) a.is_fill[(int64_t)b * a.T + t] = -1;
  }
  for (int j = threadIdx.x; j < a.Lmax; j += NT) {
    a.first[(int64_t)b * a.Lmax + j] = -1;
    a.last[(int64_t)b * a.Lmax + j] = -1;
    a.char_logp[(int64_t)b * a.Lmax + j] = 0.f;
  }
  for (int n = threadIdx.x; n < a.Nmax; n += NT) {
    a.utt_first[(int64_t)b * a.Nmax + n] = -1;
    a.utt_last[(int64_t)b * a.Nmax + n] = -1;
    a.utt_conf[(int64_t)b * a.Nmax + n] = 0.f;
    if (SKIP) a.utt_skipped[(int64_t)b * a.Nmax + n] = -1;
  }
  if (threadIdx.x == 0) {
    a.score[b] = NEG_INF;
    for (int i = 0; i < 4; ++i) a.stamps[(int64_t)b * 4 + i] = 0;   // no phases to report
  }
}

// the back-pointer of state `sh` (0 .. 63) of a 64-state group held as two 64-bit words
template <int P>
__device__ __forceinline__ int seg_code(unsigned long long w0, unsigned long long w1, int sh) {
  if (P == 1) return (int)((w0 >> sh) & 1) + 2 * (int)((w1 >> sh) & 1);
  const int pos = (sh / P) * 2 * P + (sh % P);               // the low bit; the high bit is P further, in the same word
  const unsigned long long w = pos < 64 ? w0 : w1;
  return (int)((w >> (pos & 63)) & 1) + 2 * (int)((w >> ((pos & 63) + P)) & 1);
}

// the n whose junction J_n is the blank state 2 * pos (J_0 = 0, J_n = 2 * ue[n - 1]); -1 when there is none
__device__ __forceinline__ int seg_junction(const int32_t* ue, int nu, int pos) {
  if (pos == 0) return 0;
  int lo = 0, hi = nu - 1;                                   // the first n with ue[n] >= pos: ue[nu - 1] = L >= pos
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ue[mid] < pos) lo = mid + 1;
    else hi = mid;
  }
  return ue[lo] == pos ? lo + 1 : -1;
}

template <int NT, int P, bool SKIP>
__global__ __launch_bounds__(NT) void ctc_segment_kernel(SegArgs a) {
  constexpr int LINE = 2 + NT;                               // two pads, then every thread's top value
  constexpr int NL = P == 1 ? 1 : P / 2;                     // label states of a thread's block
  extern __shared__ double seg_smem[];
  __shared__ double end_v[2];
  __shared__ int end_t[2];
  __shared__ int span[2];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int len = min(a.frame_lens[b], a.T), L = a.label_lens[b], S = 2 * L + 1, V = a.V;
  const int nu = a.n_utts[b];
  const int32_t* ue = a.utt_ends + (int64_t)b * a.utt_ld;
  bool ok = len >= 1 && L >= 1 && L <= a.Lmax && nu >= 1 && nu <= a.Nmax && nu <= L;
  int bad = 0;
  if (ok) {
    for (int n = tid; n < nu; n += NT) {
      const int e = ue[n], p = n ? ue[n - 1] : 0;
      if (e <= p || e > L || (n == nu - 1 && e != L)) bad = 1;
    }
  }
  if (__syncthreads_or(bad) || !ok) {                        // nothing to segment
    seg_none<NT, SKIP>(a, b);
    return;
  }
  const float* logits = a.logits + (int64_t)b * a.T * V;
  const int32_t* yr = a.y + (int64_t)b * a.y_ld;
  double* lse = a.lse + (int64_t)b * a.T;
  double* qv = a.q + (int64_t)b * a.T;
  double* fws = SKIP ? a.fws + (int64_t)b * a.T : nullptr;
  unsigned long long* bp = a.bp + (int64_t)b * a.T * a.groups * 2;
  int32_t* path = a.path + (int64_t)b * a.T;
  long long* stamps = a.stamps + (int64_t)b * 4;
  if (tid == 0) stamps[0] = wall_clock64();

  // the frames' normalisers, one wave per frame (ctc_table's arithmetic)
  for (int t = wave; t < len; t += NT / 64) {
    const float* row = logits + (int64_t)t * V;
    if (SKIP) {                                              // lse_t and f_t, the same over the classes that are not the
      float m = -INFINITY, m2 = -INFINITY;                   // blank, from one read of the row per pass
      for (int v = lane; v < V; v += 64) {
        const float x = row[v];
        m = fmaxf(m, x);
        if (v != a.blank) m2 = fmaxf(m2, x);
      }
      m = wave_max(m);
      m2 = wave_max(m2);
      float sum = 0.f, sum2 = 0.f;
      for (int v = lane; v < V; v += 64) {
        const float x = row[v];
        sum += expf(x - m);
        if (v != a.blank) sum2 += expf(x - m2);
      }
      sum = wave_sum(sum);
      sum2 = wave_sum(sum2);
      if (lane == 0) {
        lse[t] = (double)m + (double)logf(sum);
        fws[t] = (double)(m2 + logf(sum2)) - ((double)m + (double)logf(sum));
      }
      continue;
    }
    float m = -INFINITY;
    for (int v = lane; v < V; v += 64) m = fmaxf(m, row[v]);
    m = wave_max(m);
    float sum = 0.f;
    for (int v = lane; v < V; v += 64) sum += expf(row[v] - m);
    sum = wave_sum(sum);
    if (lane == 0) lse[t] = (double)m + (double)logf(sum);
  }
  for (int i = tid; i < 2 * LINE; i += NT) seg_smem[i] = NEG_INF;
  double* jv = seg_smem + 2 * LINE;                          // SKIP: jv[2][Nmax + 3], the junctions' values
  const int JL = a.Nmax + 3;                                 // J_0 .. J_Nmax, a slot that stays -inf, a slot nobody reads
  if (SKIP)
    for (int i = tid; i < 2 * JL; i += NT) jv[i] = NEG_INF;
  __syncthreads();
  if (tid == 0) { seg_smem[1] = 0.0; seg_smem[LINE + 1] = 0.0; }   // the virtual start state -1, in both lines
  __syncthreads();

  const int base = tid * P;
  const bool active = base < S;
  // P = 1: the thread's state is blank (even tid) or a label; P > 1: even k are blanks, odd k labels
  int col[NL];
  unsigned skip = 0;                                         // bit i: label state i of the block may take s - 2
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int s = P == 1 ? base : base + 2 * i + 1;
    const bool is_label = (s & 1) && s < S;
    col[i] = is_label ? yr[s >> 1] : a.blank;
    if (is_label && (s == 1 || yr[s >> 1] != yr[(s >> 1) - 1])) skip |= 1u << i;
  }
  // SKIP: bit i = blank state i of the block (P = 1: the thread's state) is a junction; jn0: the first one's n
  unsigned jm = 0;
  int jn0 = 0;
  if (SKIP && active) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int s = P == 1 ? base : base + 2 * i;
      if (!(s & 1) && s < S) {
        const int n = seg_junction(ue, nu, s >> 1);
        if (n >= 0) {
          if (!jm) jn0 = n;
          jm |= 1u << i;
        }
      }
    }
  }
  const int jtop = jn0 + __popc(jm) - 1;                     // the n of the block's last junction
  // the end states' running (value, frame) maximum
  const int e1 = S - 1, e2 = S - 2;
  const int k1 = e1 % P, k2 = e2 % P;                        // uniform over the workgroup
  const bool own1 = tid == e1 / P, own2 = tid == e2 / P;      // L >= 1: both exist
  double best1 = NEG_INF, best2 = NEG_INF;
  int at1 = -1, at2 = -1;

  double d[P];
#pragma unroll
  for (int k = 0; k < P; ++k) d[k] = NEG_INF;
  float xl_next[NL], xb_next = 0.f;
  double lse_next = lse[0], fw_next = SKIP ? fws[0] : 0.0;
  if (active) {
#pragma unroll
    for (int i = 0; i < NL; ++i) xl_next[i] = logits[col[i]];
    if (P > 1) xb_next = logits[a.blank];
  }
  for (int t = 0; t < len; ++t) {
    const double* prev = seg_smem + (t & 1) * LINE;
    double* cur = seg_smem + ((t + 1) & 1) * LINE;
    float xl[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) xl[i] = xl_next[i];
    const float xb = xb_next;
    const double ls = lse_next;
    const double fv = fw_next + a.fill_pen;                  // SKIP: the filler's value of this frame
    const double* jprev = jv + (t & 1) * JL;
    double* jcur = jv + ((t + 1) & 1) * JL;
    if (t + 1 < len) {
      lse_next = lse[t + 1];
      if (SKIP) fw_next = fws[t + 1];
      if (active) {
        const float* row = logits + (int64_t)(t + 1) * V;
#pragma unroll
        for (int i = 0; i < NL; ++i) xl_next[i] = row[col[i]];
        if (P > 1) xb_next = row[a.blank];
      }
    }
    unsigned lo = 0, hi = 0;
    if (active) {
      if (P == 1) {
        double best = d[0];                                  // stay wins a tie, then s - 1, then s - 2 (the start last)
        const double one = prev[1 + base];
        double two = skip ? prev[base] : NEG_INF;
        if (SKIP && jm && jn0 >= 1) two = jprev[jn0 - 1] + a.skip_pen;   // a blank has no s - 2: the skip takes its place
        if (one > best) { best = one; lo = 1; }
        if (two > best) { best = two; lo = 0; hi = 1; }
        double em = (double)xl[0] - ls;
        if (SKIP && jm) em = fv > em ? fv : em;              // the blank wins a tie
        d[0] = best + em;
        cur[2 + base] = d[0];
        if (SKIP && jm) jcur[jn0] = d[0];
      } else {
        const double l1 = prev[1 + tid];                     // state base - 1: s - 1 of k = 0 and s - 2 of k = 1
        const double lpb = (double)xb - ls;
        const double lpj = fv > lpb ? fv : lpb;              // SKIP: a junction's emission; the blank wins a tie
        // One pass over the block, downwards: d[k - 1] and d[k - 2] are still frame t - 1's.  JUNC (SKIP, and the block
        // holds a junction): every blank reads and writes the table without a branch -- a blank that is no junction, and
        // J_0, which nothing skips into, read the slot that stays -inf and write the slot that nobody reads.  Many threads
        // store to that last slot in one frame: a deliberate write-write race on a word that is never loaded.  nj: the n
        // of the junction met next on the way down.
        auto pass = [&](auto junc) {
          constexpr bool JUNC = decltype(junc)::value;
          int nj = jtop;
#pragma unroll
          for (int k = P - 1; k >= 0; --k) {
            double best = d[k];
            const double one = k >= 1 ? d[k - 1] : l1;
            if (one > best) { best = one; lo |= 1u << k; }
            if (k & 1) {
              const double two = k >= 2 ? d[k - 2] : l1;     // k = 1: state base - 1
              if (((skip >> (k >> 1)) & 1) && two > best) { best = two; lo &= ~(1u << k); hi |= 1u << k; }
              d[k] = best + ((double)xl[k >> 1] - ls);
            } else if (JUNC) {
              const bool junction = (jm >> (k >> 1)) & 1;
              const int n = nj;
              nj -= junction;
              const double two = jprev[junction && n >= 1 ? n - 1 : a.Nmax + 1] + a.skip_pen;
              if (two > best) { best = two; lo &= ~(1u << k); hi |= 1u << k; }
              d[k] = best + (junction ? lpj : lpb);
              jcur[junction ? n : a.Nmax + 2] = d[k];
            } else {
              d[k] = best + lpb;
            }
          }
        };
        if (SKIP && jm) pass(std::true_type{});
        else pass(std::false_type{});
        cur[2 + tid] = d[P - 1];
      }
      if (own1 | own2) {
        double v1 = NEG_INF, v2 = NEG_INF;
#pragma unroll
        for (int k = 0; k < P; ++k) {
          if (k == k1) v1 = d[k];
          if (k == k2) v2 = d[k];
        }
        if (own1 && v1 > best1) { best1 = v1; at1 = t; }     // strict: the earliest frame stays
        if (own2 && v2 > best2) { best2 = v2; at2 = t; }
      }
    }
    if (P == 1) {
      const unsigned long long wl = __ballot(lo), wh = __ballot(hi);
      if (lane == 0 && wave < a.groups) {
        unsigned long long* w = bp + ((int64_t)t * a.groups + wave) * 2;
        w[0] = wl;
        w[1] = wh;
      }
    } else if (active) {
      if (P == 8) reinterpret_cast<unsigned short*>(bp + (int64_t)t * a.groups * 2)[tid] = (unsigned short)(lo | (hi << 8));
      else reinterpret_cast<unsigned*>(bp + (int64_t)t * a.groups * 2)[tid] = lo | (hi << 16);
    }
    __syncthreads();
  }
  if (own1) { end_v[0] = best1; end_t[0] = at1; }
  if (own2) { end_v[1] = best2; end_t[1] = at2; }
  __syncthreads();
  // the larger value; among equals the earlier frame, then S - 1 over S - 2
  const bool second = end_v[1] > end_v[0] || (end_v[1] == end_v[0] && end_t[1] >= 0 && end_t[1] < end_t[0]);
  const double d_end = second ? end_v[1] : end_v[0];
  const int t_end = second ? end_t[1] : end_t[0];
  if (!(d_end > NEG_INF)) {                                  // the frames cannot hold the labels
    seg_none<NT, SKIP>(a, b);
    return;
  }
  if (tid == 0) stamps[1] = wall_clock64();
  int32_t* first = a.first + (int64_t)b * a.Lmax;
  int32_t* last = a.last + (int64_t)b * a.Lmax;
  if (SKIP)                                                  // a skipped utterance's labels are never visited
    for (int j = tid; j < L; j += NT) { first[j] = -1; last[j] = -1; }
  if (wave == 0) {
    int st = second ? S - 2 : S - 1;
    int t_start = 0;
    for (int t0 = t_end; t0 >= 0 && st >= 0;) {
      const int t = t0 - lane, top = st >> 6;
      unsigned long long m0[3] = {0, 0, 0}, m1[3] = {0, 0, 0};   // frame t's words of groups top, top - 1, top - 2
      if (t >= 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (top - k >= 0) {
            const unsigned long long* w = bp + ((int64_t)t * a.groups + (top - k)) * 2;
            m0[k] = w[0];
            m1[k] = w[1];
          }
      }
      int mine = -1, used = 0;
      const int n = min(64, t0 + 1);
      for (int i = 0; i < n; ++i) {                          // st falls by at most 2 per step: it stays in the three groups
        if (lane == i) mine = st;
        used = i + 1;
        const int k = top - (st >> 6);
        const unsigned long long w0 = __shfl(k == 0 ? m0[0] : k == 1 ? m0[1] : m0[2], i);
        const unsigned long long w1 = __shfl(k == 0 ? m1[0] : k == 1 ? m1[1] : m1[2], i);
        const int code = __builtin_amdgcn_readfirstlane(seg_code<P>(w0, w1, st & 63));
        if (SKIP && code == 2 && !(st & 1)) {                // the skip: from J_n to J_{n-1}, outside the groups loaded
          const int nj = seg_junction(ue, nu, st >> 1);
          st = __builtin_amdgcn_readfirstlane(nj >= 2 ? 2 * ue[nj - 2] : 0);
          break;                                             // the chunk starts again at the new state
        }
        st -= code;
        if (st < 0) {                                        // the step into the virtual state: the path starts at this frame
          t_start = t0 - i;
          break;
        }
      }
      if (t >= 0 && lane < used) path[t] = mine;             // the frames before the start are written below
      t0 -= used;
    }
    if (lane == 0) { span[0] = t_start; span[1] = t_end; }
    if (tid == 0) stamps[2] = wall_clock64();
  }
  __syncthreads();
  // derived outputs, in parallel from the path
  const int t_start = span[0];
  int32_t* fill = SKIP ? a.is_fill + (int64_t)b * a.T : nullptr;
  for (int t = tid; t < a.T; t += NT)
    if (t < t_start || t > t_end) {
      path[t] = -1;
      if (SKIP) fill[t] = -1;
    }
  float* clp = a.char_logp + (int64_t)b * a.Lmax;
  for (int j = L + tid; j < a.Lmax; j += NT) { first[j] = -1; last[j] = -1; clp[j] = 0.f; }
  for (int t = t_start + tid; t <= t_end; t += NT) {
    const int s = path[t];
    const int c = (s & 1) ? yr[s >> 1] : a.blank;
    qv[t] = (double)logits[(int64_t)t * V + c] - lse[t];
    if (SKIP) {                                              // a junction frame: the frame loop's expression again
      const double fv = fws[t] + a.fill_pen;
      const bool won = !(s & 1) && seg_junction(ue, nu, s >> 1) >= 0 && fv > qv[t];
      if (won) qv[t] = fv;
      fill[t] = won;
    }
    if (s & 1) {
      if (t == t_start || path[t - 1] != s) first[s >> 1] = t;
      if (t == t_end || path[t + 1] != s) last[s >> 1] = t;
    }
  }
  if (tid == 0) a.score[b] = d_end;
  __syncthreads();
  for (int j = tid; j < L; j += NT) {
    double acc = 0.0;
    const int hi_t = min(last[j], t_end);
    for (int t = max(first[j], t_start); t <= hi_t; ++t) acc += qv[t];
    clp[j] = (float)acc;
  }
  // Kuerzinger's min-mean, one wave per utterance: lane i sums blocks i, i + 64, .. of `window` frames in frame order
  int32_t* uf = a.utt_first + (int64_t)b * a.Nmax;
  int32_t* ul = a.utt_last + (int64_t)b * a.Nmax;
  float* uc = a.utt_conf + (int64_t)b * a.Nmax;
  int32_t* us = SKIP ? a.utt_skipped + (int64_t)b * a.Nmax : nullptr;
  for (int n = nu + tid; n < a.Nmax; n += NT) {
    uf[n] = -1; ul[n] = -1; uc[n] = 0.f;
    if (SKIP) us[n] = -1;
  }
  for (int n = wave; n < nu; n += NT / 64) {
    if (SKIP) {                                              // aligned whole or skipped whole: its first label tells
      const bool skipped = first[n ? ue[n - 1] : 0] < 0;
      if (lane == 0) us[n] = skipped;
      if (skipped) {
        if (lane == 0) { uf[n] = -1; ul[n] = -1; uc[n] = 0.f; }
        continue;
      }
    }
    const int f = max(first[n ? ue[n - 1] : 0], t_start), l = min(last[ue[n] - 1], t_end);
    double worst = INFINITY;
    for (int64_t t0 = (int64_t)f + (int64_t)lane * a.window; t0 <= l; t0 += (int64_t)64 * a.window) {
      const int t1 = (int)min((int64_t)l, t0 + a.window - 1);
      double acc = 0.0;
      for (int t = (int)t0; t <= t1; ++t) acc += qv[t];
      worst = fmin(worst, acc / (double)(t1 - (int)t0 + 1));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) worst = fmin(worst, __shfl_xor(worst, off));
    if (lane == 0) { uf[n] = f; ul[n] = l; uc[n] = (float)worst; }
  }
  if (tid == 0) stamps[3] = wall_clock64();
}

struct SegForm { int sp_max, threads, per_thread; };
constexpr SegForm SEG_FORMS[] = {{256, 256, 1},   {512, 512, 1},   {1024, 1024, 1}, {2048, 256, 8},
                                 {4096, 512, 8}, {8192, 1024, 8}, {16384, 1024, 16}};
constexpr int SEG_N_FORMS = sizeof(SEG_FORMS) / sizeof(SEG_FORMS[0]);

int seg_form(int64_t T, int64_t Lmax) {
  if (T < 1 || T > SEG_MAX_T || Lmax < 1 || 2 * Lmax + 1 > SEG_MAX_STATES) return -1;
  for (int f = 0; f < SEG_N_FORMS; ++f)
    if (2 * Lmax + 1 <= SEG_FORMS[f].sp_max) return f;
  return -1;
}

int64_t seg_groups(int64_t Lmax) { return (2 * Lmax + 1 + 63) / 64; }

int seg_check_shape(int64_t B, int64_t T, int64_t V, int64_t Lmax, int64_t Nmax) {
  if (B < 1 || B > 65535 || V < 2 || V > SEG_MAX_V || Nmax < 1 || Nmax > Lmax) return SSASR_EARG;
  return seg_form(T, Lmax) < 0 ? SSASR_EARG : SSASR_OK;
}

}  // namespace

extern "C" int ssasr_ctc_segment_form(int64_t T, int64_t Lmax, int* threads, int* states_per_thread) {
  const int f = seg_form(T, Lmax);
  if (f < 0) return -1;
  if (threads) *threads = SEG_FORMS[f].threads;
  if (states_per_thread) *states_per_thread = SEG_FORMS[f].per_thread;
  return f;
}

namespace {

template <bool SKIP>
void (*seg_fn(const SegForm& form))(SegArgs) {
  if (form.per_thread == 1)
    return form.threads == 256 ? ctc_segment_kernel<256, 1, SKIP> : form.threads == 512 ? ctc_segment_kernel<512, 1, SKIP>
                                                                                         : ctc_segment_kernel<1024, 1, SKIP>;
  if (form.per_thread == 8)
    return form.threads == 256 ? ctc_segment_kernel<256, 8, SKIP> : form.threads == 512 ? ctc_segment_kernel<512, 8, SKIP>
                                                                                         : ctc_segment_kernel<1024, 8, SKIP>;
  return ctc_segment_kernel<1024, 16, SKIP>;
}

constexpr int SEG_SKIP_MAX_UTTS = 1024;                      // the LDS table of junction values: 2 x (1,024 + 3) doubles

// ssasr_ctc_segment (skip false: no penalties, no utt_skipped, no is_fill) and ssasr_ctc_segment_skip
int seg_run(bool skip, const float* logits, const int32_t* frame_lens, const int32_t* y, int64_t y_ld,
            const int32_t* label_lens, const int32_t* utt_ends, int64_t utt_ld, const int32_t* n_utts, int64_t B,
            int64_t T, int64_t V, int64_t Lmax, int64_t Nmax, int64_t window, int blank, double skip_penalty,
            double fill_penalty, void* ws, int64_t ws_bytes, int32_t* path, int32_t* first, int32_t* last,
            float* char_logp, double* score, int32_t* utt_first, int32_t* utt_last, float* utt_conf,
            int32_t* utt_skipped, int32_t* is_fill, void* stream) {
  if (!logits || !frame_lens || !y || !label_lens || !utt_ends || !n_utts || !ws || !path || !first || !last ||
      !char_logp || !score || !utt_first || !utt_last || !utt_conf)
    return SSASR_EARG;
  if (skip && (!utt_skipped || !is_fill || Nmax > SEG_SKIP_MAX_UTTS || !(skip_penalty <= 0) || !(fill_penalty <= 0)))
    return SSASR_EARG;                                       // !(x <= 0): a positive value, +inf or a NaN
  if (seg_check_shape(B, T, V, Lmax, Nmax) != SSASR_OK || blank < 0 || blank >= V) return SSASR_EARG;
  if (window < 1 || window > INT32_MAX || y_ld < Lmax || utt_ld < Nmax) return SSASR_EARG;
  const int64_t need = skip ? ssasr_ctc_segment_skip_ws_bytes(B, T, V, Lmax, Nmax) : ssasr_ctc_segment_ws_bytes(B, T, V, Lmax, Nmax);
  if ((reinterpret_cast<uintptr_t>(ws) & 7) || need <= 0 || ws_bytes < need) return SSASR_EARG;
  SegArgs a{};
  a.logits = logits; a.frame_lens = frame_lens; a.y = y; a.y_ld = y_ld; a.label_lens = label_lens;
  a.utt_ends = utt_ends; a.utt_ld = utt_ld; a.n_utts = n_utts;
  a.T = (int)T; a.V = (int)V; a.Sp = (int)(2 * Lmax + 1); a.Lmax = (int)Lmax; a.Nmax = (int)Nmax;
  a.window = (int)window; a.blank = blank;
  a.groups = (int)seg_groups(Lmax);
  a.lse = reinterpret_cast<double*>(ws);
  a.q = a.lse + B * T;
  double* next = a.q + B * T;
  if (skip) {
    a.fws = next;
    next += B * T;
  }
  a.bp = reinterpret_cast<unsigned long long*>(next);
  a.stamps = reinterpret_cast<long long*>(a.bp + B * T * a.groups * 2);
  a.path = path; a.first = first; a.last = last; a.char_logp = char_logp; a.score = score;
  a.utt_first = utt_first; a.utt_last = utt_last; a.utt_conf = utt_conf;
  a.utt_skipped = utt_skipped; a.is_fill = is_fill; a.skip_pen = skip_penalty; a.fill_pen = fill_penalty;
  const SegForm form = SEG_FORMS[seg_form(T, Lmax)];
  const size_t lds = (size_t)2 * (2 + form.threads) * 8 + (skip ? (size_t)2 * (Nmax + 3) * 8 : 0);
  void (*fn)(SegArgs) = skip ? seg_fn<true>(form) : seg_fn<false>(form);
  hipLaunchKernelGGL(fn, dim3((unsigned)B), dim3(form.threads), lds, (hipStream_t)stream, a);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}

}  // namespace

extern "C" int64_t ssasr_ctc_segment_skip_ws_bytes(int64_t B, int64_t T, int64_t V, int64_t Lmax, int64_t Nmax) {
  if (seg_check_shape(B, T, V, Lmax, Nmax) != SSASR_OK || Nmax > SEG_SKIP_MAX_UTTS) return 0;
  return B * T * 24 + B * T * seg_groups(Lmax) * 16 + B * 32;   // lse, q and f, back-pointers, stamps
}

extern "C" int64_t ssasr_ctc_segment_ws_bytes(int64_t B, int64_t T, int64_t V, int64_t Lmax, int64_t Nmax) {
  if (seg_check_shape(B, T, V, Lmax, Nmax) != SSASR_OK) return 0;
  return B * T * 16 + B * T * seg_groups(Lmax) * 16 + B * 32;   // lse and q, back-pointers, stamps
}

extern "C" int ssasr_ctc_segment(const float* logits, const int32_t* frame_lens, const int32_t* y, int64_t y_ld,
                                 const int32_t* label_lens, const int32_t* utt_ends, int64_t utt_ld,
                                 const int32_t* n_utts, int64_t B, int64_t T, int64_t V, int64_t Lmax, int64_t Nmax,
                                 int64_t window, int blank, void* ws, int64_t ws_bytes, int32_t* path, int32_t* first,
                                 int32_t* last, float* char_logp, double* score, int32_t* utt_first, int32_t* utt_last,
                                 float* utt_conf, void* stream) {
  return seg_run(false, logits, frame_lens, y, y_ld, label_lens, utt_ends, utt_ld, n_utts, B, T, V, Lmax, Nmax, window,
                 blank, 0.0, 0.0, ws, ws_bytes, path, first, last, char_logp, score, utt_first, utt_last, utt_conf,
                 nullptr, nullptr, stream);
}

extern "C" int ssasr_ctc_segment_skip(const float* logits, const int32_t* frame_lens, const int32_t* y, int64_t y_ld,
                                      const int32_t* label_lens, const int32_t* utt_ends, int64_t utt_ld,
                                      const int32_t* n_utts, int64_t B, int64_t T, int64_t V, int64_t Lmax,
                                      int64_t Nmax, int64_t window, int blank, const double* skip_penalty,
                                      const double* fill_penalty, void* ws, int64_t ws_bytes, int32_t* path, int32_t* first,
                                      int32_t* last, float* char_logp, double* score, int32_t* utt_first,
                                      int32_t* utt_last, float* utt_conf, int32_t* utt_skipped, int32_t* is_fill,
                                      void* stream) {
  if (!skip_penalty || !fill_penalty) return SSASR_EARG;     // host memory, read here
  return seg_run(true, logits, frame_lens, y, y_ld, label_lens, utt_ends, utt_ld, n_utts, B, T, V, Lmax, Nmax, window,
                 blank, *skip_penalty, *fill_penalty, ws, ws_bytes, path, first, last, char_logp, score, utt_first,
                 utt_last, utt_conf, utt_skipped, is_fill, stream);
}
