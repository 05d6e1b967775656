// The edit-distance sweep shared by score.hip (ssasr_edit_score) and mbr.hip (ssasr_mbr_select).
//
// A cell is ONE 32-bit word, dist << 16 | S, so that one unsigned min takes the lexicographic minimum of
// (S + D + I, S).  The sweep runs over anti-diagonals: a thread owns reference column j; at step d it computes cell
// (d - j, j) from its own value of step d - 1 and column j - 1's values of steps d - 1 and d - 2.  The neighbour's
// value comes by a one-lane DPP shift of the whole wave; across a wave boundary it comes through a two-slot LDS
// exchange and one __syncthreads() per step (kBarrier).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace editdp {

constexpr int MAX_WAVES = 16;         // of a block: one exchange slot per wave and parity

// lane l's value <- lane l - 1's, over the whole wave; lane 0 gets 0 (DPP wave_shr:1)
__device__ __forceinline__ uint32_t lane_shr1(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false);
}

// exclusive prefix sum of one flag per lane over the wave; total: the wave's count
__device__ __forceinline__ int wave_scan_flag(bool f, int& total) {
  const unsigned long long b = __ballot(f);
  total = __popcll(b);
  return __popcll(b & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// The packed cell (H, R) of hyp[0 .. H) against ref[0 .. R), valid in the thread whose column j == R.
//   j      the thread's column: its index inside the run of consecutive waves that sweeps this pair.  Columns
//          j > R compute nothing (R == -1: a wave that has no pair and only keeps the barriers' company).
//   steps  the number of anti-diagonals to run, >= H + R; cells past the pair's own H + R are masked.
// kBarrier false: the columns fit ONE wave; no barrier, no LDS exchange; steps may be the pair's own H + R.
// kBarrier true:  EVERY thread of the block must call with the SAME steps (one __syncthreads() before the loop and
//   one per step); lane 63 of every wave publishes its cell in xch[parity][wave] and lane 0 of a wave with `chained`
//   set takes the cell of wave - 1 (`wave` is the index inside the block).
template <typename T, bool kBarrier>
__device__ __forceinline__ uint32_t sweep(const T* ref, int R, const T* hyp, int H, int j, int steps,
                                          uint32_t (*xch)[MAX_WAVES], int wave, bool chained) {
  const int lane = threadIdx.x & 63;
  uint32_t mine = 0;                          // step 0: cell (0, 0) = 0 in column 0
  uint32_t left1 = 0, left2 = 0;
  const T rt = ref[j >= 1 && j <= R ? j - 1 : 0];
  const int hlast = H > 0 ? H - 1 : 0;
  if (kBarrier) {
    if (lane == 63) xch[0][wave] = mine;
    __syncthreads();
  }
  T hn = hyp[min(max(-j, 0), hlast)];         // hyp[i - 1] of step 1
  for (int d = 1; d <= steps; ++d) {
    uint32_t in = lane_shr1(mine);
    if (kBarrier && lane == 0 && chained) in = xch[(d - 1) & 1][wave - 1];
    left2 = left1;
    left1 = in;
    const T hc = hn;
    const int i = d - j;
    hn = hyp[min(max(i, 0), hlast)];          // the next step's token, loaded a step ahead
    if (j <= R && i >= 0 && i <= H) {
      uint32_t v;
      if (j == 0) v = (uint32_t)i << 16;
      else if (i == 0) v = (uint32_t)j << 16;
      else v = min(min(left2 + (hc != rt ? 0x10001u : 0u), mine + 0x10000u), left1 + 0x10000u);
      mine = v;
    }
    if (kBarrier) {
      if (lane == 63) xch[d & 1][wave] = mine;
      __syncthreads();
    }
  }
  return mine;
}

}  // namespace editdp
