// The CTC prefix beam search, written once: the frame body of ctc_prefix_beam_kernel, ctc_prefix_beam_graph_kernel
// (ctc.hip) and ctc_prefix_beam_lm_kernel (infer.hip).  BUILD-DEFINED (include/ssasr.h, "CTC-only decoding").
//
// One workgroup of NT threads per utterance, a serial loop over its frames.  Per beam member the search keeps g_b / g_n
// in double, the text's length, last character and a rolling hash of the text and of its parent in LDS (State), and the
// texts themselves in the workspace, one block per beam (B_{t-1} is read, B_t written).  A frame is: the row's
// log-softmax (wave 0, the next row's logits loaded one frame ahead); each member's parent looked up among the members
// (length and hash as a filter, then the characters, one wave per member); the K + K V candidate keys into LDS, an
// extension that is itself a member being no candidate; K rounds of a block-wide argmax; the winners' scalars and
// texts written to the other beam; the term's hook.  After the last frame the totals are formed, ranked by counting
// and written out.
//
// A Term is what a kernel adds to a candidate's key beside the CTC total (DESIGN.md 4.19 has the contract):
//   kScored      false: nothing (NoTerm); true: the term derives from Scored, its Mem from ScoredMem
//   Mem          what the term keeps in LDS, a member of State: per-member scalars [2][kMaxK] and rows [slot][64]
//   init(m, V)   the empty text's state and rows; runs before the barrier that opens the first frame
//   step(m, cur, u, c)         what extension c of member u adds to the member's accumulated score (double)
//   keep(m, cur, nxt, j, w)    winner j is the kept member w: copy the term's own per-member scalars
//   inherit(m, cur, nxt, j, u, c)   winner j is the new text u.c
//   after_commit(s, cur, nxt, K, V) block-wide, once the winners' scalars, slots and texts are written and a barrier
//                has passed: fills the rows of the frame's new members (s.tm.ext[0 .. n_ext)) at their slots.  The
//                next frame's two barriers lie before step's first read of them; end is called after the last
//                frame's hook with no barrier between, so a term whose end reads rows ends its hook with a barrier
//   has_end(), end(m, cur, j)  the end term of member j
// The variant is the template argument: no run-time branch on it.  g_b / g_n stay pure CTC masses under every term.
#pragma once
#include "common.h"

#include <cmath>

namespace ctc_prefix {

constexpr int kMaxK = 32;       // beam members
constexpr int kMaxV = 64;       // classes: one wave holds a row
constexpr int kMaxT = 4096;     // frames
constexpr int kMaxB = 65535;    // utterances: the grid
constexpr unsigned long long kHashMul = 0x9E3779B97F4A7C15ull;
constexpr double kNegInf = -INFINITY;

inline bool shape_ok(int64_t B, int64_t T, int64_t V, int64_t K) {
  return B >= 1 && B <= kMaxB && T >= 1 && T <= kMaxT && V >= 2 && V <= kMaxV && K >= 1 && K <= kMaxK;
}

// what the three kernels take in common
struct Args {
  const float* logits;       // [B][T][V]
  const int32_t* frame_lens; // [B]
  int T, V, K, blank;
  int32_t* text;             // [B][2][K][T] the two beams' texts
  int32_t* chars;            // [B][K][T]
  int32_t* n_chars;          // [B][K]
  float* scores;             // [B][K]
  int32_t* n_hyps;           // [B]
};

inline Args make_args(const float* logits, const int32_t* frame_lens, int64_t T, int64_t V, int64_t K, int blank,
                      void* text, int32_t* chars, int32_t* n_chars, float* scores, int32_t* n_hyps) {
  return Args{logits, frame_lens, (int)T, (int)V, (int)K, blank, reinterpret_cast<int32_t*>(text), chars, n_chars,
              scores, n_hyps};
}

// log(exp(a) + exp(b)): double operands, exp and log in float on the difference from the larger one
__device__ __forceinline__ double lae(double a, double b) {
  const double m = fmax(a, b), n = fmin(a, b);
  if (n == kNegInf) return m;
  return m + (double)logf(1.f + expf((float)(n - m)));
}

struct NoMem {};

// what a scored term keeps per member, and the bookkeeping of its rows
struct ScoredMem {
  double acc[2][kMaxK];                  // the term's score of the member's text
  int slot[2][kMaxK];                    // the member's row slot: kept while the member stays in the beam
  int ext[kMaxK], n_ext;                 // the frame's winners that are new extensions
  float fctc[kMaxK], fext[kMaxK];        // the final CTC and term parts
};

// the weights a scored term brings; `on` false: the term is unread (weight 0), acc stays 0
struct Scored {
  static constexpr bool kScored = true;
  bool on, use_len;
  double weight, beta;                   // the term's weight, the length bonus
  float *ctc_scores, *term_scores;       // [B][K] the extra output columns
};

struct NoTerm {
  static constexpr bool kScored = false;
  using Mem = NoMem;
  __device__ void init(Mem&, int) {}
  template <class S>
  __device__ void after_commit(S&, int, int, int, int) {}
};

template <int NT, class Term>
struct State {
  double gb[2][kMaxK], gn[2][kMaxK];                     // the two beams' members
  unsigned long long hs[2][kMaxK], hp[2][kMaxK];         // hash of the text, of the text's parent
  double lpd[kMaxV];                                     // the frame's log-softmax
  double sgb[kMaxK], sgn[kMaxK];                         // g_b', g_n' of the kept texts
  double tot[kMaxK + kMaxK * kMaxV];                     // the candidates' keys: [K] kept, then [K][V] extensions
  double wv[2][NT / 64];
  int wi[2][NT / 64], win[kMaxK];
  int tlen[2][kMaxK], tlast[2][kMaxK];                   // length, last character (-1: the empty text)
  int par[kMaxK];                                        // the member that is this member's parent, -1: none
  float fkey[kMaxK], ftot[kMaxK];                        // the final ranking
  int fsrc[kMaxK];
  signed char child[kMaxK * kMaxV];                      // [u][c]: the member that is u.c, -1: none
  typename Term::Mem tm;
};

// phase 1: the frame's log-softmax (ctc_table's normaliser) by wave 0, the next row loaded one frame ahead
template <int NT, class Term>
__device__ __forceinline__ void frame_log_softmax(State<NT, Term>& s, const float* logits, int t, int len, int V,
                                                  int K, float& x_next) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < K * V; i += NT) s.child[i] = -1;
  if (wave == 0) {
    const float x = x_next;
    if (t + 1 < len && lane < V) x_next = logits[(int64_t)(t + 1) * V + lane];
    const float m = wave_max(x);
    const float sum = wave_sum(lane < V ? expf(x - m) : 0.f);
    const double lse = (double)m + (double)logf(sum);
    if (lane < V) s.lpd[lane] = (double)x - lse;
  }
}

// phase 2: each member's parent among the members: a lane per possible parent filters, the wave compares the characters
template <int NT, class Term>
__device__ __forceinline__ void parent_lookup(State<NT, Term>& s, const int32_t* told, int cur, int n, int T, int V) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int w = wave; w < n; w += NT / 64) {
    const int lw = s.tlen[cur][w];
    int found = -1;
    if (lw >= 1) {
      unsigned long long mask = __ballot(lane < n && s.tlen[cur][lane < n ? lane : 0] == lw - 1 &&
                                         s.hs[cur][lane < n ? lane : 0] == s.hp[cur][w]);
      while (mask != 0 && found < 0) {                       // at most n turns
        const int u = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        int differ = 0;
        for (int i = lane; i < lw - 1; i += 64) differ |= told[(int64_t)w * T + i] != told[(int64_t)u * T + i];
        if (!__any(differ)) found = u;
      }
      if (lane == 0 && found >= 0) s.child[found * V + s.tlast[cur][w]] = (signed char)w;
    }
    if (lane == 0) s.par[w] = found;
  }
}

// the CTC total of extension c of member u: also the new member's g_n'
template <int NT, class Term>
__device__ __forceinline__ double extension_total(const State<NT, Term>& s, int cur, int u, int c) {
  return s.lpd[c] + (s.tlast[cur][u] == c ? s.gb[cur][u] : lae(s.gb[cur][u], s.gn[cur][u]));
}

// phase 3: the candidates' keys: the CTC total, + weight (acc + step) + length_bonus |text| under a scored term; each
// thread remembers the best of its own
template <int NT, class Term>
__device__ __forceinline__ void candidate_keys(State<NT, Term>& s, const Term& term, int cur, int n, int K, int V,
                                               int blank, double& best, int& bidx) {
  const int tid = threadIdx.x, ncand = K + K * V;
  const double lpb = s.lpd[blank];
  best = kNegInf;
  bidx = INT32_MAX;
  for (int idx = tid; idx < ncand; idx += NT) {
    double v = kNegInf;
    if (idx < K) {
      const int w = idx;
      if (w < n) {
        const double nb = lpb + lae(s.gb[cur][w], s.gn[cur][w]);
        double nn = kNegInf;
        const int c = s.tlast[cur][w];
        if (c >= 0) {
          const int p = s.par[w];
          double via = kNegInf;
          if (p >= 0) via = s.tlast[cur][p] == c ? s.gb[cur][p] : lae(s.gb[cur][p], s.gn[cur][p]);
          nn = s.lpd[c] + lae(s.gn[cur][w], via);
        }
        s.sgb[w] = nb;
        s.sgn[w] = nn;
        v = lae(nb, nn);
        if constexpr (Term::kScored) {
          if (v > kNegInf) {
            if (term.on) v += term.weight * s.tm.acc[cur][w];
            if (term.use_len) v += term.beta * (double)s.tlen[cur][w];
          }
        }
      }
    } else {
      const int u = (idx - K) / V, c = (idx - K) % V;
      if (u < n && c != blank && s.child[u * V + c] < 0) {
        v = extension_total(s, cur, u, c);
        if constexpr (Term::kScored) {
          if (v > kNegInf) {                                 // a forbidden step (-inf) leaves no candidate
            if (term.on) v += term.weight * (s.tm.acc[cur][u] + term.step(s.tm, cur, u, c));
            if (term.use_len) v += term.beta * (double)(s.tlen[cur][u] + 1);
          }
        }
      }
    }
    s.tot[idx] = v;
    if (v > best) { best = v; bidx = idx; }
  }
}

// phase 4: B_t: K rounds of a block-wide argmax (the lowest index among equals), the winner leaving the pool.
// -> the number of winners; s.win holds them after the caller's barrier.
template <int NT, class Term>
__device__ __forceinline__ int select_winners(State<NT, Term>& s, int K, int V, double best, int bidx) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, ncand = K + K * V;
  int n_new = 0;
  for (int r = 0; r < K; ++r) {
    double m = best;
    int mi = bidx;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double om = __shfl_xor(m, off);
      const int oi = __shfl_xor(mi, off);
      if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
    }
    if (lane == 0) { s.wv[r & 1][wave] = m; s.wi[r & 1][wave] = mi; }
    __syncthreads();
    double gm = s.wv[r & 1][0];
    int gi = s.wi[r & 1][0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) {
      const double om = s.wv[r & 1][w];
      const int oi = s.wi[r & 1][w];
      if (om > gm || (om == gm && oi < gi)) { gm = om; gi = oi; }
    }
    if (!(gm > kNegInf)) break;                              // fewer finite candidates than K
    if (tid == 0) s.win[r] = gi;
    n_new = r + 1;
    if (gi % NT == tid) {
      s.tot[gi] = kNegInf;
      best = kNegInf;
      bidx = INT32_MAX;
      for (int idx = tid; idx < ncand; idx += NT) {
        const double v = s.tot[idx];
        if (v > best) { best = v; bidx = idx; }
      }
    }
  }
  return n_new;
}

// phase 5: the winners become B_t: scalars, then texts.  A new extension's g_n' is its CTC total, formed again (under
// a scored term the key is no longer that total); a scored term's new members take a slot no kept member holds and
// are listed in ext[].
template <int NT, class Term>
__device__ __forceinline__ void commit_winners(State<NT, Term>& s, Term& term, const int32_t* told, int32_t* tnew,
                                               int cur, int n_new, int K, int V, int T) {
  const int tid = threadIdx.x, nxt = cur ^ 1;
  if (tid < n_new) {
    const int w = s.win[tid];
    if (w < K) {
      s.gb[nxt][tid] = s.sgb[w]; s.gn[nxt][tid] = s.sgn[w];
      s.hs[nxt][tid] = s.hs[cur][w]; s.hp[nxt][tid] = s.hp[cur][w];
      s.tlen[nxt][tid] = s.tlen[cur][w]; s.tlast[nxt][tid] = s.tlast[cur][w];
      if constexpr (Term::kScored) {
        s.tm.acc[nxt][tid] = s.tm.acc[cur][w]; s.tm.slot[nxt][tid] = s.tm.slot[cur][w];
        term.keep(s.tm, cur, nxt, tid, w);
      }
    } else {
      const int u = (w - K) / V, c = (w - K) % V;
      s.gb[nxt][tid] = kNegInf;
      s.gn[nxt][tid] = extension_total(s, cur, u, c);
      if constexpr (Term::kScored) {
        s.tm.acc[nxt][tid] = term.on ? s.tm.acc[cur][u] + term.step(s.tm, cur, u, c) : 0.0;
        term.inherit(s.tm, cur, nxt, tid, u, c);
      }
      s.hs[nxt][tid] = s.hs[cur][u] * kHashMul + (unsigned long long)(c + 1); s.hp[nxt][tid] = s.hs[cur][u];
      s.tlen[nxt][tid] = s.tlen[cur][u] + 1; s.tlast[nxt][tid] = c;
    }
  }
  if constexpr (Term::kScored) {
    if (tid == 0) {                                          // slots: the kept members' stay taken, the rest is free
      unsigned used = 0;
      for (int j = 0; j < n_new; ++j)
        if (s.win[j] < K) used |= 1u << s.tm.slot[cur][s.win[j]];
      int ne = 0;
      for (int j = 0; j < n_new; ++j)
        if (s.win[j] >= K) {
          const int sl = __ffs((int)~used) - 1;              // K members at most: a bit below K is clear
          used |= 1u << sl;
          s.tm.slot[nxt][j] = sl;
          s.tm.ext[ne++] = j;
        }
      s.tm.n_ext = ne;
    }
  }
  for (int j = 0; j < n_new; ++j) {
    const int w = s.win[j];
    const int src = w < K ? w : (w - K) / V;
    const int l = s.tlen[cur][src];                          // l <= t < T: the appended character stays in the row
    for (int i = tid; i < l; i += NT) tnew[(int64_t)j * T + i] = told[(int64_t)src * T + i];
    if (w >= K && tid == 0) tnew[(int64_t)j * T + l] = (w - K) % V;
  }
}

// phase 6: the totals with the end term, ranked by counting as rescore_kernel ranks, and the outputs.  Without a term
// the members are in the order they won, which is this order: the totals are non-increasing in double, hence in
// float, and ties go to the lower index.
template <int NT, class Term>
__device__ __forceinline__ void rank_and_emit(State<NT, Term>& s, const Term& term, const Args& a, const int32_t* tfin,
                                              int cur, int n) {
  const int b = blockIdx.x, tid = threadIdx.x, K = a.K, T = a.T;
  if (tid < K) {
    float key = -INFINITY, total = -INFINITY, ctc = -INFINITY, part = 0.f;
    if (tid < n) {
      const double c = lae(s.gb[cur][tid], s.gn[cur][tid]);
      double l = 0.0, tv = c;
      if constexpr (Term::kScored) {
        if (term.on) {
          l = s.tm.acc[cur][tid];
          tv += term.weight * l;
        }
        if (term.use_len) tv += term.beta * (double)s.tlen[cur][tid];
        if (term.on && term.has_end()) {
          const double e = term.end(s.tm, cur, tid);
          l += e;
          tv += term.weight * e;
        }
      }
      total = (float)tv; ctc = (float)c; part = (float)l;
      key = total != total ? -INFINITY : total;
    }
    s.fkey[tid] = key; s.ftot[tid] = total;
    if constexpr (Term::kScored) { s.tm.fctc[tid] = ctc; s.tm.fext[tid] = part; }
    s.fsrc[tid] = -1;
  }
  __syncthreads();
  if (tid < n) {
    const float key = s.fkey[tid];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += (s.fkey[j] > key || (s.fkey[j] == key && j < tid)) ? 1 : 0;
    s.fsrc[rank] = tid;
  }
  __syncthreads();
  for (int j = 0; j < K; ++j) {
    const int src = s.fsrc[j];
    const int l = src >= 0 ? s.tlen[cur][src] : 0;
    int32_t* out = a.chars + ((int64_t)b * K + j) * T;
    for (int i = tid; i < T; i += NT) out[i] = i < l ? tfin[(int64_t)src * T + i] : 0;
  }
  if (tid < K) {
    const int src = s.fsrc[tid];
    const int64_t o = (int64_t)b * K + tid;
    a.n_chars[o] = src >= 0 ? s.tlen[cur][src] : 0;
    a.scores[o] = src >= 0 ? s.ftot[src] : -INFINITY;
    if constexpr (Term::kScored) {
      term.ctc_scores[o] = src >= 0 ? s.tm.fctc[src] : -INFINITY;
      term.term_scores[o] = src >= 0 ? s.tm.fext[src] : 0.f;
    }
  }
  if (tid == 0) a.n_hyps[b] = n;
}

// the search of utterance blockIdx.x: set-up, the frame loop over the phases, the emit
template <int NT, class Term>
__device__ __forceinline__ void search(const Args& a, Term& term, State<NT, Term>& s) {
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int len = max(min(a.frame_lens[b], a.T), 0), V = a.V, K = a.K, T = a.T;
  const float* logits = a.logits + (int64_t)b * T * V;
  int32_t* text = a.text + (int64_t)b * 2 * K * T;
  int n = 1, cur = 0;
  if (tid == 0) {                                            // B_0: the empty text
    s.gb[0][0] = 0.0; s.gn[0][0] = kNegInf;
    s.hs[0][0] = 0; s.hp[0][0] = 0;
    s.tlen[0][0] = 0; s.tlast[0][0] = -1;
    if constexpr (Term::kScored) { s.tm.acc[0][0] = 0.0; s.tm.slot[0][0] = 0; }
  }
  float x_next = (wave == 0 && lane < V && len > 0) ? logits[lane] : -INFINITY;
  term.init(s.tm, V);
  __syncthreads();
  for (int t = 0; t < len; ++t) {
    const int32_t* told = text + (int64_t)cur * K * T;
    int32_t* tnew = text + (int64_t)(cur ^ 1) * K * T;
    frame_log_softmax(s, logits, t, len, V, K, x_next);
    __syncthreads();
    parent_lookup(s, told, cur, n, T, V);
    __syncthreads();
    double best;
    int bidx;
    candidate_keys(s, term, cur, n, K, V, a.blank, best, bidx);
    const int n_new = select_winners(s, K, V, best, bidx);
    __syncthreads();
    commit_winners(s, term, told, tnew, cur, n_new, K, V, T);
    __syncthreads();
    term.after_commit(s, cur, cur ^ 1, K, V);
    cur ^= 1;
    n = n_new;
  }
  rank_and_emit(s, term, a, text + (int64_t)cur * K * T, cur, n);
}

}  // namespace ctc_prefix
