// Edit-distance scoring of decoded hypotheses against reference labels (BUILD-DEFINED; include/ssasr.h,
// ssasr_edit_score): character and word substitution / deletion / insertion counts of P (hypothesis, reference)
// pairs in one launch, one workgroup per pair.
//
// The metric is the lexicographic minimum of (S + D + I, S) over all alignments, so it is exact and has no
// traversal-order dependence: a cell is ONE 32-bit word, dist << 16 | S, and one unsigned min compares the pair
// (dist <= 8191 + 1023 and S <= 1023 both fit 16 bits).  With I - D = H - R the counts follow from the last cell.
//
// Stages, per pair:
//   1. compaction: ids < first_char are dropped (pads, <sos>, <eos>); a block-wide prefix sum over ballots writes
//      the kept tokens of reference and hypothesis into one LDS array, and a second sum numbers the word starts
//      (maximal runs of non-space tokens, str.split()) and writes each word's [start, end).
//   2. word ids: word w of the concatenation (reference words, then hypothesis words) gets the smallest index of
//      an equal word -- lengths, then tokens; exact, no hashing; one thread per word.
//   3. the DP, once over the tokens and once over the word ids, by one templated routine: an anti-diagonal sweep,
//      thread j owning reference column j.  At step d it computes cell (d - j, j) from its own value of step d - 1
//      and thread j - 1's values of steps d - 1 and d - 2 (edit_dp.h, shared with mbr.hip).  The neighbour's value
//      comes by a one-lane DPP shift of the whole wave (no LDS round trip); across a wave boundary it comes through
//      a two-slot LDS exchange and one __syncthreads() per step.  A pair whose columns fit one wave runs the sweep
//      in wave 0 with no barrier.
// Every thread reaches every barrier: all loop bounds are the pair's lengths, which are uniform over the block.
#include "common.h"
#include "edit_dp.h"
#include "../../include/ssasr.h"

namespace {

constexpr int SCORE_MAX_R = 1023;     // reference tokens per row, before dropping: R + 1 columns <= 1024 threads
constexpr int SCORE_MAX_H = 8191;     // hypothesis tokens per row, before dropping
constexpr int SCORE_MAX_WAVES = editdp::MAX_WAVES;

struct ScoreArgs {
  const int32_t* hyp;
  const int32_t* hyp_lens;
  const int32_t* ref;
  const int32_t* ref_lens;
  const int32_t* ref_of;
  int64_t hyp_ld, ref_ld;
  int Hmax, Rmax, first_char, space;
  int32_t* out;
};

struct ScoreShared {
  int wave_tot[SCORE_MAX_WAVES];
  uint32_t xch[2][SCORE_MAX_WAVES];
};

__host__ __device__ inline int score_max_words(int Hmax, int Rmax) { return (Hmax + 1) / 2 + (Rmax + 1) / 2; }

// exclusive prefix sum of one flag per thread over the block; total: the block's count.  Two barriers.
__device__ __forceinline__ int block_scan_flag(bool f, int* wave_tot, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const unsigned long long b = __ballot(f);
  const int pre = __popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0) wave_tot[wave] = __popcll(b);
  __syncthreads();
  int off = 0, tot = 0;
  for (int w = 0; w < nwaves; ++w) {
    const int v = wave_tot[w];
    off += w < wave ? v : 0;
    tot += v;
  }
  __syncthreads();
  total = tot;
  return off + pre;
}

// the tokens >= first_char of src[0 .. len) -> dst, in order; returns their number (uniform over the block)
__device__ int score_compact(const int32_t* src, int len, int first_char, int32_t* dst, int* wave_tot) {
  int n = 0;
  for (int base = 0; base < len; base += blockDim.x) {
    const int i = base + threadIdx.x;
    const int tok = i < len ? src[i] : 0;
    const bool keep = i < len && tok >= first_char;
    int tot;
    const int pos = block_scan_flag(keep, wave_tot, tot);
    if (keep) dst[n + pos] = tok;
    n += tot;
  }
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(n);
}

// the words of tok[off .. off + n): word wbase + k gets wse[2 (wbase + k)] = its first position and
// wse[2 (wbase + k) + 1] = one past its last, both as indices into tok; returns the number of words
__device__ int score_words(const int32_t* tok, int off, int n, int space, int wbase, unsigned short* wse,
                           int* wave_tot) {
  int nw = 0;
  for (int base = 0; base < n; base += blockDim.x) {
    const int i = base + threadIdx.x;
    const bool in = i < n;
    const bool word = in && tok[off + i] != space;
    const bool st = word && (i == 0 || tok[off + i - 1] == space);
    const bool en = word && (i == n - 1 || tok[off + i + 1] == space);
    int tot;
    const int before = block_scan_flag(st, wave_tot, tot);          // word starts at positions < i
    if (st) wse[2 * (wbase + nw + before)] = (unsigned short)(off + i);
    if (en) wse[2 * (wbase + nw + before + (st ? 1 : 0) - 1) + 1] = (unsigned short)(off + i + 1);
    nw += tot;
  }
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(nw);
}

// The packed cell (H, R) of hyp[0 .. H) against ref[0 .. R), valid in thread R (R + 1 <= blockDim.x): editdp::sweep
// over the block's columns, with the barrier when they span more than one wave, else in wave 0 alone.
template <typename T>
__device__ uint32_t score_dp(const T* ref, int R, const T* hyp, int H, uint32_t (*xch)[SCORE_MAX_WAVES]) {
  const int j = threadIdx.x, wave = j >> 6;
  if (R >= 64) return editdp::sweep<T, true>(ref, R, hyp, H, j, H + R, xch, wave, wave > 0);    // uniform
  if (wave == 0) return editdp::sweep<T, false>(ref, R, hyp, H, j, H + R, xch, 0, false);
  return 0;
}

// S, D, I, N from the last cell
__device__ __forceinline__ void score_store(int32_t* out, uint32_t cell, int H, int R) {
  const int dist = (int)(cell >> 16), S = (int)(cell & 0xffffu);
  out[0] = S;
  out[1] = (dist - S - H + R) / 2;
  out[2] = (dist - S + H - R) / 2;
  out[3] = R;
}

__global__ __launch_bounds__(1024) void edit_score_kernel(ScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char score_lds[];
  __shared__ ScoreShared sh;
  const int64_t p = blockIdx.x;
  int32_t* tok = reinterpret_cast<int32_t*>(score_lds);                               // [Rmax + Hmax + 1]
  unsigned short* wse = reinterpret_cast<unsigned short*>(tok + a.Rmax + a.Hmax + 1);  // [2 (words + 1)]
  unsigned short* wid = wse + 2 * (score_max_words(a.Hmax, a.Rmax) + 1);              // [words + 1]

  const int64_t r = a.ref_of ? a.ref_of[p] : p;
  const int rl = __builtin_amdgcn_readfirstlane(min(max(a.ref_lens[r], 0), a.Rmax));
  const int hl = __builtin_amdgcn_readfirstlane(min(max(a.hyp_lens[p], 0), a.Hmax));
  const int hoff = a.Rmax;
  // slots that a sweep may read for an empty sequence
  if (threadIdx.x == 0) {
    tok[0] = 0;
    tok[hoff] = 0;
  }
  __syncthreads();

  // 1. compaction and word boundaries
  const int R = score_compact(a.ref + r * a.ref_ld, rl, a.first_char, tok, sh.wave_tot);
  const int H = score_compact(a.hyp + p * a.hyp_ld, hl, a.first_char, tok + hoff, sh.wave_tot);
  const int RW = score_words(tok, 0, R, a.space, 0, wse, sh.wave_tot);
  const int HW = score_words(tok, hoff, H, a.space, RW, wse, sh.wave_tot);

  // 2. word ids
  const int W = RW + HW;
  for (int w = threadIdx.x; w < W; w += blockDim.x) {
    const int s = wse[2 * w], len = wse[2 * w + 1] - s;
    int id = w;
    for (int v = 0; v < w; ++v) {
      const int sv = wse[2 * v];
      if (wse[2 * v + 1] - sv != len) continue;
      int k = 0;
      while (k < len && tok[sv + k] == tok[s + k]) ++k;
      if (k == len) {
        id = v;
        break;
      }
    }
    wid[w] = (unsigned short)id;
  }
  if (threadIdx.x == 0) wid[W] = 0;
  __syncthreads();

  // 3. the two sweeps
  int32_t* out = a.out + p * 8;
  const uint32_t cc = score_dp<int32_t>(tok, R, tok + hoff, H, sh.xch);
  if ((int)threadIdx.x == R) score_store(out, cc, H, R);
  __syncthreads();
  const uint32_t cw = score_dp<unsigned short>(wid, RW, wid + RW, HW, sh.xch);
  if ((int)threadIdx.x == RW) score_store(out + 4, cw, HW, RW);
}

}  // namespace

extern "C" int ssasr_edit_score(const int32_t* hyp, int64_t hyp_ld, const int32_t* hyp_lens, const int32_t* ref,
                                int64_t ref_ld, const int32_t* ref_lens, const int32_t* ref_of, int64_t P,
                                int64_t Hmax, int64_t Rmax, int32_t first_char, int32_t space, int32_t* out,
                                void* stream) {
  if (P < 0 || P > INT32_MAX || Hmax < 0 || Hmax > SCORE_MAX_H || Rmax < 0 || Rmax > SCORE_MAX_R) return SSASR_EARG;
  if (hyp_ld < Hmax || ref_ld < Rmax) return SSASR_EARG;
  if (P == 0) return SSASR_OK;
  if ((!hyp && Hmax > 0) || (!ref && Rmax > 0) || !hyp_lens || !ref_lens || !out) return SSASR_EARG;
  ScoreArgs a{};
  a.hyp = hyp; a.hyp_lens = hyp_lens; a.ref = ref; a.ref_lens = ref_lens; a.ref_of = ref_of;
  a.hyp_ld = hyp_ld; a.ref_ld = ref_ld; a.Hmax = (int)Hmax; a.Rmax = (int)Rmax;
  a.first_char = first_char; a.space = space; a.out = out;
  const int nt = 64 * (int)((Rmax + 1 + 63) / 64);
  const size_t lds = (size_t)(Rmax + Hmax + 1) * 4 + (size_t)(score_max_words(a.Hmax, a.Rmax) + 1) * 6;
  SSASR_HIP(hipFuncSetAttribute((const void*)edit_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(edit_score_kernel, dim3((unsigned)P), dim3(nt), lds, (hipStream_t)stream, a);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}
