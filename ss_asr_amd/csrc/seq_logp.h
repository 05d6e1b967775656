// One step of a teacher-forced row's log-probability, logP_r = sum over labelled t of (z[t][lab] - lse_t) (include/ssasr.h,
// "MWER training"): the label rule, the wave's log-sum-exp in double and the step's term.  Shared by the MWER loss
// (mwer.hip) and the n-best rescoring (rescore.hip), so that both form the same bits from the same logits.
#pragma once
#include "common.h"

constexpr int SEQ_REG = 4;         // logits a lane keeps in registers: rows of V <= 256 are read once

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// the label of step t of a row, 0 (unlabelled) for a column past y_cols and for an id that names no class
__device__ __forceinline__ int seq_label(const int32_t* yr, int t, int y_cols, int V) {
  const int lab = t + 1 < y_cols ? yr[t + 1] : 0;
  return lab > 0 && lab < V ? lab : 0;
}

// lse = (double)max + log(sum exp((double)z - max)) of the V logits at `row` (unit stride), formed by a whole wave, in
// every lane.  The step's term of logP is then (double)row[lab] - lse.
__device__ __forceinline__ double seq_step_lse(const float* row, int V, int lane) {
  float z[SEQ_REG];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < SEQ_REG; ++i) {
    const int v = lane + 64 * i;
    z[i] = v < V ? row[v] : -INFINITY;
    m = fmaxf(m, z[i]);
  }
  for (int v = lane + 64 * SEQ_REG; v < V; v += 64) m = fmaxf(m, row[v]);
  m = wave_max(m);
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < SEQ_REG; ++i)
    if (lane + 64 * i < V) s += exp((double)z[i] - (double)m);
  for (int v = lane + 64 * SEQ_REG; v < V; v += 64) s += exp((double)row[v] - (double)m);
  s = wave_sum_f64(s);
  return (double)m + log(s);
}

__device__ __forceinline__ double seq_step_term(const float* row, int lab, double lse) { return (double)row[lab] - lse; }
