// Minimum-Bayes-risk selection over an n-best list or a set of samples (BUILD-DEFINED; include/ssasr.h,
// ssasr_mbr_select): the pairwise character and word edit distances of an utterance's K hypotheses, the set's
// posterior, every candidate's expected distance and the candidate that minimises it, in one launch, one workgroup
// per utterance.
//
// Stages, per utterance (tokens, words and the metric are score.hip's; the sweep is edit_dp.h's):
//   1. compaction, a WAVE per hypothesis: ids < first_char are dropped by a ballot prefix sum, the kept tokens of
//      hypothesis k go to tok[k * Hmax ..]; a second pass numbers the word starts and writes each word's
//      [start, end) into hypothesis k's slice of the word table (slot k * WH + i, WH = (Hmax + 1) / 2).  Done once
//      per hypothesis, whatever number of pairs it is part of.
//   2. word ids, a thread per word: the smallest slot of an equal word among ALL the utterance's words -- lengths,
//      then tokens; exact, no hashing.
//   3. the unordered pairs (k, j < k) of the set, once over the tokens and once over the word ids.  With L the
//      longest sequence of the utterance, the block's waves form groups of G = ceil((L + 1) / 64) waves and the groups
//      take the pairs round-robin; the thread that owns the last cell writes pair[k][j] and pair[j][k].
//   4. posterior, risks and argmin: a lane per candidate, everything in double, sums in the order j = 0 .. K - 1.
//
// Barriers.  Every __syncthreads() of this file is reached by every thread of the block:
//   - stages 1, 2 and 4 and the G == 1 form of stage 3 have loops whose trip counts differ between waves (a wave's
//     own hypotheses, words or pairs, a pair's own lengths).  NONE of them contains a barrier: a wave works alone
//     there (ballots and DPP shifts only), and the barriers stand between the stages, outside every loop and branch.
//   - the G > 1 form of stage 3 exchanges cells across waves with one barrier per step.  Its two loops are bounded
//     by `rounds` (pairs / groups, rounded up) and `steps` = 2 L, both functions of the utterance alone and hence
//     uniform over the block; a group whose pair is shorter, or that has no pair left, or a wave outside every group
//     runs the same steps with its cells masked (R = -1 masks them all).  G itself is uniform, so the whole block
//     takes the same form.
#include "common.h"
#include "edit_dp.h"
#include "../../include/ssasr.h"

#include <cmath>

namespace {

constexpr int MBR_MAX_K = 32;
constexpr int MBR_MAX_H = 1023;       // both sides of a pair are columns: L + 1 <= 1024 threads
constexpr int MBR_MAX_TOK = 8192;     // K * Hmax: the kept tokens of an utterance, 32 KB of LDS

struct MbrArgs {
  const int32_t* chars;
  const int32_t* n_chars;
  const int32_t* n_hyps;
  const float* scores;
  int64_t hyp_ld;
  int K, Hmax, first_char, space, unit, posterior;
  float scale;
  int32_t* best;
  float* risk;
  int32_t* pair;
};

struct MbrShared {
  double x[MBR_MAX_K];                // scale * score, -inf where that is not finite; then the risks
  double p[MBR_MAX_K];
  int len[MBR_MAX_K];                 // kept tokens
  int nw[MBR_MAX_K];                  // words
  uint32_t xch[2][editdp::MAX_WAVES];
  unsigned short dsel[MBR_MAX_K * MBR_MAX_K];     // the distances of the chosen unit
};

// pair p = k (k - 1) / 2 + j, j < k  ->  (k, j)
__device__ __forceinline__ void mbr_pair_of(int p, int& k, int& j) {
  int kk = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)p)) * 0.5f);
  while (kk * (kk - 1) / 2 > p) --kk;
  while ((kk + 1) * kk / 2 <= p) ++kk;
  k = kk;
  j = p - kk * (kk - 1) / 2;
}

// Stage 3 for one unit: seq + k * stride holds sequence k, len[k] its length, L the longest of the set.
template <typename T>
__device__ void mbr_pairs(const T* seq, int stride, const int* len, int nh, int L, int unit, const MbrArgs& a,
                          int64_t n, MbrShared& sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int G = (L + 1 + 63) >> 6;              // waves per pair; uniform; <= nwaves as L <= Hmax
  const int ngroups = nwaves / G;
  const int g = wave / G;
  const int P = nh * (nh - 1) / 2;
  const int K = a.K;
  int32_t* out = a.pair + n * K * K * 2 + unit;
  if (G == 1) {
    // a wave per pair, no barrier inside: the bounds are the wave's own
    for (int p = wave; p < P; p += nwaves) {
      int k, j;
      mbr_pair_of(p, k, j);
      const int R = len[j], H = len[k];
      const uint32_t cell = editdp::sweep<T, false>(seq + j * stride, R, seq + k * stride, H, lane, H + R, sh.xch, 0,
                                                    false);
      if (lane == R) {
        const int dist = (int)(cell >> 16);
        out[(k * K + j) * 2] = dist;
        out[(j * K + k) * 2] = dist;
        if (unit == a.unit) sh.dsel[k * K + j] = sh.dsel[j * K + k] = (unsigned short)dist;
      }
    }
  } else {
    // uniform bounds: see the header comment
    const int rounds = (P + ngroups - 1) / ngroups;
    const int steps = 2 * L;
    const int col = (int)threadIdx.x - g * G * 64;
    for (int r = 0; r < rounds; ++r) {
      const int p = r * ngroups + g;
      const bool have = g < ngroups && p < P;
      int k = 0, j = 0;
      if (have) mbr_pair_of(p, k, j);
      const int R = have ? len[j] : -1, H = have ? len[k] : 0;
      const uint32_t cell = editdp::sweep<T, true>(seq + j * stride, R, seq + k * stride, H, col, steps, sh.xch, wave,
                                                   wave - g * G > 0);
      if (have && col == R) {
        const int dist = (int)(cell >> 16);
        out[(k * K + j) * 2] = dist;
        out[(j * K + k) * 2] = dist;
        if (unit == a.unit) sh.dsel[k * K + j] = sh.dsel[j * K + k] = (unsigned short)dist;
      }
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(1024) void mbr_select_kernel(MbrArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mbr_lds[];
  __shared__ MbrShared sh;
  const int64_t n = blockIdx.x;
  const int K = a.K, Hmax = a.Hmax, WH = (Hmax + 1) / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  int32_t* tok = reinterpret_cast<int32_t*>(mbr_lds);                            // [K * Hmax + 1]
  unsigned short* wse = reinterpret_cast<unsigned short*>(tok + K * Hmax + 1);   // [2 (K * WH + 1)]
  unsigned short* wid = wse + 2 * (K * WH + 1);                                  // [K * WH + 1]
  const int nh = __builtin_amdgcn_readfirstlane(min(max(a.n_hyps[n], 0), K));

  // what stage 3 does not write: rows and columns outside the set, and the diagonal
  for (int e = threadIdx.x; e < K * K; e += blockDim.x) {
    const int k = e / K, j = e - k * K;
    const bool inside = k < nh && j < nh;
    if (!inside || k == j) {
      int32_t* o = a.pair + (n * K * K + e) * 2;
      o[0] = o[1] = inside ? 0 : -1;
      sh.dsel[e] = 0;
    }
  }

  // 1. compaction and word boundaries, a wave per hypothesis; no barrier inside the loops
  for (int k = wave; k < K; k += nwaves) {
    int kept = 0;
    if (k < nh) {
      const int len = min(max(a.n_chars[n * K + k], 0), Hmax);
      const int32_t* src = a.chars + (n * K + k) * a.hyp_ld;
      int32_t* dst = tok + k * Hmax;
      for (int base = 0; base < len; base += 64) {
        const int i = base + lane;
        const int t = i < len ? src[i] : 0;
        const bool keep = i < len && t >= a.first_char;
        int tot;
        const int pos = editdp::wave_scan_flag(keep, tot);
        if (keep) dst[kept + pos] = t;
        kept += tot;
      }
    }
    if (lane == 0) sh.len[k] = kept;
  }
  __syncthreads();
  for (int k = wave; k < K; k += nwaves) {
    const int cnt = sh.len[k], off = k * Hmax, wb = k * WH;
    int nw = 0;
    for (int base = 0; base < cnt; base += 64) {
      const int i = base + lane;
      const bool word = i < cnt && tok[off + i] != a.space;
      const bool st = word && (i == 0 || tok[off + i - 1] == a.space);
      const bool en = word && (i == cnt - 1 || tok[off + i + 1] == a.space);
      int tot;
      const int before = editdp::wave_scan_flag(st, tot);          // word starts at positions < i
      if (st) wse[2 * (wb + nw + before)] = (unsigned short)(off + i);
      if (en) wse[2 * (wb + nw + before + (st ? 1 : 0) - 1) + 1] = (unsigned short)(off + i + 1);
      nw += tot;
    }
    if (lane == 0) sh.nw[k] = nw;
  }
  __syncthreads();
  int L = 0, LW = 0;
  for (int k = 0; k < nh; ++k) {
    L = max(L, sh.len[k]);
    LW = max(LW, sh.nw[k]);
  }
  L = __builtin_amdgcn_readfirstlane(L);
  LW = __builtin_amdgcn_readfirstlane(LW);

  // 2. word ids: slot k * WH + i is word i of hypothesis k
  for (int w = threadIdx.x; w < nh * WH; w += blockDim.x) {
    const int k = w / WH, i = w - k * WH;
    if (i >= sh.nw[k]) continue;
    const int s = wse[2 * w], len = wse[2 * w + 1] - s;
    int id = w;
    for (int kv = 0; kv <= k && id == w; ++kv) {
      const int nv = kv == k ? i : sh.nw[kv];
      for (int iv = 0; iv < nv; ++iv) {
        const int v = kv * WH + iv, sv = wse[2 * v];
        if (wse[2 * v + 1] - sv != len) continue;
        int c = 0;
        while (c < len && tok[sv + c] == tok[s + c]) ++c;
        if (c == len) {
          id = v;
          break;
        }
      }
    }
    wid[w] = (unsigned short)id;
  }
  __syncthreads();

  // 3. every unordered pair once, over the tokens and over the word ids
  mbr_pairs<int32_t>(tok, Hmax, sh.len, nh, L, 0, a, n, sh);
  mbr_pairs<unsigned short>(wid, WH, sh.nw, nh, LW, 1, a, n, sh);

  // 4. posterior, risks, argmin: thread k is candidate k
  const int k = threadIdx.x;
  if (k < K) {
    double x = -INFINITY;
    if (a.posterior == 0 && k < nh) {
      x = (double)a.scale * (double)a.scores[n * K + k];
      if (!std::isfinite(x)) x = -INFINITY;
    }
    sh.x[k] = x;
  }
  __syncthreads();
  if (k < K) {
    double m = -INFINITY;
    for (int j = 0; j < nh; ++j) m = fmax(m, sh.x[j]);
    double p = nh > 0 ? 1.0 / (double)nh : 0.0;                 // the uniform posterior, also when nothing is finite
    if (m > -INFINITY) {
      double sum = 0.0;
      for (int j = 0; j < nh; ++j) sum += exp(sh.x[j] - m);     // exp(-inf) = 0
      p = exp(sh.x[k] - (m + log(sum)));
    }
    sh.p[k] = k < nh ? p : 0.0;
  }
  __syncthreads();
  double risk = INFINITY;
  if (k < nh) {
#pragma clang fp contract(off)                                  // products and sums rounded one by one, as the host does
    double acc = 0.0;
    for (int j = 0; j < nh; ++j) {
      const double term = sh.p[j] * (double)sh.dsel[k * K + j];
      acc = acc + term;
    }
    risk = acc;
  }
  if (k < K) a.risk[n * K + k] = (float)risk;
  __syncthreads();                                              // sh.x is read above by every candidate
  if (k < K) sh.x[k] = risk;
  __syncthreads();
  if (k == 0) {
    int b = -1;
    double lowest = INFINITY;
    for (int j = 0; j < nh; ++j)
      if (b < 0 || sh.x[j] < lowest) {
        b = j;
        lowest = sh.x[j];
      }
    a.best[n] = b;
  }
}

}  // namespace

extern "C" int ssasr_mbr_select(const int32_t* chars, int64_t hyp_ld, const int32_t* n_chars, const int32_t* n_hyps,
                                const float* scores, int64_t N, int64_t K, int64_t Hmax, int32_t first_char,
                                int32_t space, int unit, int posterior, float scale, int32_t* best, float* risk,
                                int32_t* pair, void* stream) {
  if (N < 0 || N > 65535 || K < 1 || K > MBR_MAX_K || Hmax < 0 || Hmax > MBR_MAX_H || K * Hmax > MBR_MAX_TOK)
    return SSASR_EARG;
  if (hyp_ld < Hmax || (unit != 0 && unit != 1) || (posterior != 0 && posterior != 1)) return SSASR_EARG;
  if (!std::isfinite(scale) || scale < 0.0f) return SSASR_EARG;
  if (N == 0) return SSASR_OK;
  if (!n_chars || !n_hyps || !best || !risk || !pair || (!chars && Hmax > 0) || (!scores && posterior == 0))
    return SSASR_EARG;
  MbrArgs a{};
  a.chars = chars; a.n_chars = n_chars; a.n_hyps = n_hyps; a.scores = scores; a.hyp_ld = hyp_ld;
  a.K = (int)K; a.Hmax = (int)Hmax; a.first_char = first_char; a.space = space; a.unit = unit;
  a.posterior = posterior; a.scale = scale; a.best = best; a.risk = risk; a.pair = pair;
  // enough waves for the longest pair, and as many as there are pairs to run side by side
  const int pairs = (int)(K * (K - 1) / 2), wide = (int)((Hmax + 1 + 63) / 64);
  const int nwaves = std::min(std::max(std::max(wide, std::min(pairs, editdp::MAX_WAVES)), 1), editdp::MAX_WAVES);
  const int WH = (int)((Hmax + 1) / 2);
  const size_t lds = (size_t)(K * Hmax + 1) * 4 + (size_t)(K * WH + 1) * 6;
  SSASR_HIP(hipFuncSetAttribute((const void*)mbr_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(mbr_select_kernel, dim3((unsigned)N), dim3(64 * nwaves), lds, (hipStream_t)stream, a);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}
