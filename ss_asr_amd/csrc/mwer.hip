// Minimum word error rate training (BUILD-DEFINED; include/ssasr.h, "MWER training"): the expected-risk loss over
// groups of teacher-forced rows with its backward, the packing of an n-best list into teacher / label rows, and the
// row repeat that hands one encoder output to the M rows of its group.  All HBM-bound streaming work: the loss reads
// [R][U][V] logits once going forward and once going back.
//
// Loss, forward:
//   1. mwer_rows_kernel, grid (R, MWER_G) x 256 threads: ce_fwd_body<true>'s wave-per-step pass.  A wave holds its
//      step's logits in registers (V <= 256; longer rows are read again, from cache), forms the log-sum-exp in double
//      and adds (double)z[lab] - lse into the block's share of the row's log-probability.
//   2. mwer_groups_kernel, ONE block of 256 threads: a wave per group, a lane per candidate (M <= 33 <= 64).  logP_k in
//      block order, the softmax over the set in double with the maximum subtracted, the expected risk, and each row's
//      sequence-level weight w_r = ce_w[r] - (1 / G) p_r (risk_r - Rbar_g), which is all the backward needs
//      (ssasr_mwer_loss_fwd_ex, posterior 1: p_k = 1 / |S_g| instead of the softmax, the rest unchanged).  Then the
//      block sums the groups' contributions: thread t takes groups t, t + 256, ... in order, the 256 partial sums are
//      added in index order by thread 0.  No atomics: the same bits every run.
// Backward: mwer_bwd_kernel, a wave per (r, t) step: unlabelled steps are stored as zeros without a load.
#include "seq_logp.h"
#include "../../include/ssasr.h"

namespace {

constexpr int MWER_G = 8;          // blocks per row: steps t = g, g + MWER_G, ... (four waves each)
constexpr int MWER_MAX_M = 33;     // candidates per group: a beam of 32 and the reference row

// The workspace: doubles first -- logP [R], p [R], w [R], Rbar [G], the groups' CE terms [G], per-block shares
// [R][MWER_G], the log-sum-exp [R][U] as the backward reads it -- then lse [R][U] as float.
struct MwerWs {
  double* logp;
  double* phat;
  double* wgt;
  double* rbar;
  double* ce;
  double* part;
  double* lse64;
  float* lse;
};

__host__ __device__ inline MwerWs mwer_ws(void* ws, int64_t G, int64_t M, int64_t U) {
  const int64_t R = G * M;
  MwerWs w;
  w.logp = static_cast<double*>(ws);
  w.phat = w.logp + R;
  w.wgt = w.phat + R;
  w.rbar = w.wgt + R;
  w.ce = w.rbar + G;
  w.part = w.ce + G;
  w.lse64 = w.part + R * MWER_G;
  w.lse = reinterpret_cast<float*>(w.lse64 + R * U);
  return w;
}

__global__ __launch_bounds__(256) void mwer_rows_kernel(const float* logits, const int32_t* y, int64_t y_ld,
                                                        int y_cols, int U, int V, float* lse, double* lse64,
                                                        double* part) {
  __shared__ double sm[4];
  const int r = blockIdx.x, g = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int32_t* yr = y + (int64_t)r * y_ld;
  double acc = 0.0;                    // lane 0: sum over this wave's labelled steps of z[lab] - lse
  for (int t = g + MWER_G * wave; t < U; t += 4 * MWER_G) {
    const float* row = logits + ((int64_t)r * U + t) * V;
    const double ld = seq_step_lse(row, V, lane);
    const int lab = seq_label(yr, t, y_cols, V);
    if (lane == 0) {
      lse[(int64_t)r * U + t] = (float)ld;          // the correctly rounded value, as the LS kernel saves it
      lse64[(int64_t)r * U + t] = ld;               // what the backward normalises by: a step's dlogits then sum to 0
      if (lab != 0) acc += seq_step_term(row, lab, ld);
    }
  }
  if (lane == 0) sm[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[(int64_t)r * MWER_G + g] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

__global__ __launch_bounds__(256) void mwer_groups_kernel(MwerWs w, const int32_t* n_hyps, const int32_t* counts,
                                                          const float* ce_w, int G, int M, int unit, int uniform,
                                                          float* risk_out, float* loss) {
  __shared__ double s_risk[256], s_ce[256];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double inv_g = 1.0 / (double)G;
  for (int g = wave; g < G; g += 4) {
    const int n = min(max(n_hyps[g], 0), M);
    const int64_t r = (int64_t)g * M + lane;
    const bool row = lane < M, in = lane < n;
    double lp = 0.0, risk = 0.0, cw = 0.0;
    if (row) {
      for (int k = 0; k < MWER_G; ++k) lp += w.part[r * MWER_G + k];
      const int32_t* c = counts + r * 8 + (unit ? 4 : 0);
      risk = (double)c[0] + (double)c[1] + (double)c[2];
      cw = ce_w ? (double)ce_w[r] : 0.0;
    }
    const double mx = wave_max_f64(in ? lp : -INFINITY);
    const double e = in ? exp(lp - mx) : 0.0;              // an empty set: every e is 0 and nothing below divides
    const double z = wave_sum_f64(e);
    // uniform: the Monte-Carlo form, every member of a set of samples weighs 1 / |S|, whatever logP is
    const double p = in ? (uniform ? 1.0 / (double)n : e / z) : 0.0;
    const double rbar = wave_sum_f64(in ? p * risk : 0.0);
    const double ce = wave_sum_f64(row ? cw * -lp : 0.0);
    if (row) {
      w.logp[r] = lp;
      w.phat[r] = p;
      w.wgt[r] = cw - inv_g * p * (risk - rbar);           // p == 0 outside the set: the weight is ce_w alone
    }
    if (lane == 0) {
      w.rbar[g] = rbar;
      risk_out[g] = (float)rbar;
      w.ce[g] = ce;
    }
  }
  __syncthreads();
  double a = 0.0, b = 0.0;
  for (int g = threadIdx.x; g < G; g += 256) {
    a += w.rbar[g];
    b += w.ce[g];
  }
  s_risk[threadIdx.x] = a;
  s_ce[threadIdx.x] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    a = 0.0;
    b = 0.0;
    for (int i = 0; i < 256; ++i) {
      a += s_risk[i];
      b += s_ce[i];
    }
    *loss = (float)(a * inv_g + b);
  }
}

// four (r, t) steps per block, a wave each; dlogits = dloss w_r (p_v - [v == lab]) in double, rounded once
__global__ __launch_bounds__(256) void mwer_bwd_kernel(const float* logits, const int32_t* y, int64_t y_ld, int y_cols,
                                                       const double* lse, const double* wgt, const float* dloss,
                                                       int64_t steps, int U, int V, float* dlogits) {
  const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (s >= steps) return;
  const int64_t r = s / U;
  const int t = (int)(s - r * U);
  const int lab = seq_label(y + r * y_ld, t, y_cols, V);
  float* out = dlogits + s * V;
  if (lab == 0) {
    for (int v = lane; v < V; v += 64) out[v] = 0.f;
    return;
  }
  const float* row = logits + s * V;
  const double c = (double)(*dloss) * wgt[r], l = lse[s];
  for (int v = lane; v < V; v += 64) out[v] = (float)(c * (exp((double)row[v] - l) - (v == lab ? 1.0 : 0.0)));
}

// One row of the teacher / label matrix per block (64 threads); see ssasr_mwer_pack.
__global__ __launch_bounds__(64) void mwer_pack_kernel(const int32_t* chars, const int32_t* n_chars,
                                                       const int32_t* n_hyps, const int32_t* y_ref, int64_t ref_ld,
                                                       int ref_cols, int K, int steps, int eos, int L, int32_t* rows,
                                                       int32_t* hyp_lens) {
  const int64_t r = blockIdx.x;
  const int64_t n = r / (K + 1);
  const int k = (int)(r - n * (K + 1)), lane = threadIdx.x;
  int32_t* dst = rows + r * L;
  if (k == K) {
    const int32_t* src = y_ref + n * ref_ld;
    int cnt = 0;
    for (int j = lane; j < L; j += 64) {
      const int32_t v = j < ref_cols ? src[j] : 0;
      dst[j] = v;
      cnt += v != 0 ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) hyp_lens[r] = max(cnt - 1, 0);
    return;
  }
  const bool live = k < min(max(n_hyps[n], 0), K);
  const int len = live ? min(max(n_chars[n * K + k], 0), steps) : 0;
  const int32_t* src = chars + (n * K + k) * (int64_t)steps;
  for (int j = lane; j < L; j += 64) {
    int32_t v = 0;
    if (live && j >= 1 && j <= len) v = src[j - 1];
    if (live && j == len + 1) v = eos;
    dst[j] = v;
  }
  if (lane == 0) hyp_lens[r] = len;
}

// 32-bit words: dst[g * M + k][i] = src[g][i].  grid (ceil(n / 1024), G), 256 threads, four words each.
__global__ __launch_bounds__(256) void rows_repeat_fwd_kernel(const uint32_t* src, int M, int64_t n, bool vec,
                                                              uint32_t* dst) {
  const int64_t g = blockIdx.y, i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  const uint32_t* s = src + g * n + i;
  uint32_t* d = dst + g * M * n + i;
  if (vec) {
    const uint4 v = *reinterpret_cast<const uint4*>(s);
    for (int k = 0; k < M; ++k) *reinterpret_cast<uint4*>(d + k * n) = v;
  } else {
    for (int j = 0; j < 4 && i + j < n; ++j) {
      const uint32_t v = s[j];
      for (int k = 0; k < M; ++k) d[k * n + j] = v;
    }
  }
}

// dsrc[g][i] = ddst[g * M][i] + ddst[g * M + 1][i] + ... in float, k ascending: one owner per output, no atomics
__global__ __launch_bounds__(256) void rows_repeat_bwd_kernel(const float* ddst, int M, int64_t n, bool vec,
                                                              float* dsrc) {
  const int64_t g = blockIdx.y, i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  const float* s = ddst + g * M * n + i;
  float* d = dsrc + g * n + i;
  if (vec) {
    float4 a = *reinterpret_cast<const float4*>(s);
    for (int k = 1; k < M; ++k) {
      const float4 v = *reinterpret_cast<const float4*>(s + k * n);
      a.x += v.x;
      a.y += v.y;
      a.z += v.z;
      a.w += v.w;
    }
    *reinterpret_cast<float4*>(d) = a;
  } else {
    for (int j = 0; j < 4 && i + j < n; ++j) {
      float a = s[j];
      for (int k = 1; k < M; ++k) a += s[k * n + j];
      d[j] = a;
    }
  }
}

bool mwer_shape_ok(int64_t G, int64_t M, int64_t U, int64_t V) {
  return G >= 0 && M >= 1 && M <= MWER_MAX_M && G * M <= 65535 && U > 0 && V > 0 && U <= INT32_MAX && V <= INT32_MAX;
}

bool repeat_shape_ok(int64_t G, int64_t M, int64_t n) {
  return G >= 0 && G <= 65535 && M >= 1 && M <= 65535 && n > 0 && (n + 1023) / 1024 <= INT32_MAX;
}

bool aligned16(const void* a, const void* b) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}

}  // namespace

extern "C" int64_t ssasr_mwer_ws_bytes(int64_t G, int64_t M, int64_t U) {
  if (G < 0 || M < 1 || M > MWER_MAX_M || G * M > 65535 || U <= 0 || U > INT32_MAX) return 0;
  const int64_t R = G * M;
  return 8 * (3 * R + 2 * G + R * MWER_G + R * U) + 8 * ((R * U + 1) / 2);
}

extern "C" int ssasr_mwer_loss_fwd_ex(const float* logits, const int32_t* y, int64_t y_ld, int64_t y_cols,
                                   const int32_t* n_hyps, const int32_t* counts, int unit, const float* ce_w,
                                   int64_t G, int64_t M, int64_t U, int64_t V, void* ws, int64_t ws_bytes,
                                   float* risk_out, float* loss, int posterior, void* stream) {
  if (!mwer_shape_ok(G, M, U, V) || (posterior != 0 && posterior != 1) || (unit != 0 && unit != 1) || !loss)
    return SSASR_EARG;
  hipStream_t st = (hipStream_t)stream;
  if (G == 0) {
    SSASR_HIP(hipMemsetAsync(loss, 0, sizeof(float), st));
    return SSASR_OK;
  }
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 7) != 0 || ws_bytes < ssasr_mwer_ws_bytes(G, M, U)) return SSASR_EARG;
  if (!logits || !y || !n_hyps || !counts || !risk_out || y_cols < U + 1 || y_ld < y_cols || y_cols > INT32_MAX)
    return SSASR_EARG;
  const MwerWs w = mwer_ws(ws, G, M, U);
  hipLaunchKernelGGL(mwer_rows_kernel, dim3((unsigned)(G * M), MWER_G), dim3(256), 0, st, logits, y, y_ld, (int)y_cols,
                     (int)U, (int)V, w.lse, w.lse64, w.part);
  hipLaunchKernelGGL(mwer_groups_kernel, dim3(1), dim3(256), 0, st, w, n_hyps, counts, ce_w, (int)G, (int)M, unit,
                     posterior, risk_out, loss);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}

extern "C" int ssasr_mwer_loss_fwd(const float* logits, const int32_t* y, int64_t y_ld, int64_t y_cols,
                                   const int32_t* n_hyps, const int32_t* counts, int unit, const float* ce_w,
                                   int64_t G, int64_t M, int64_t U, int64_t V, void* ws, int64_t ws_bytes,
                                   float* risk_out, float* loss, void* stream) {
  return ssasr_mwer_loss_fwd_ex(logits, y, y_ld, y_cols, n_hyps, counts, unit, ce_w, G, M, U, V, ws, ws_bytes, risk_out,
                                loss, 0, stream);
}

extern "C" int ssasr_mwer_loss_bwd(const float* logits, const int32_t* y, int64_t y_ld, int64_t y_cols, int64_t G,
                                   int64_t M, int64_t U, int64_t V, const void* ws, int64_t ws_bytes,
                                   const float* dloss, float* dlogits, void* stream) {
  if (!mwer_shape_ok(G, M, U, V)) return SSASR_EARG;
  if (G == 0) return SSASR_OK;
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 7) != 0 || ws_bytes < ssasr_mwer_ws_bytes(G, M, U)) return SSASR_EARG;
  if (!logits || !y || !dloss || !dlogits || y_cols < U + 1 || y_ld < y_cols || y_cols > INT32_MAX) return SSASR_EARG;
  const int64_t steps = G * M * U;
  if ((steps + 3) / 4 > INT32_MAX) return SSASR_EARG;
  const MwerWs w = mwer_ws(const_cast<void*>(ws), G, M, U);
  hipLaunchKernelGGL(mwer_bwd_kernel, dim3((unsigned)((steps + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, y,
                     y_ld, (int)y_cols, w.lse64, w.wgt, dloss, steps, (int)U, (int)V, dlogits);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}

extern "C" int ssasr_mwer_pack(const int32_t* chars, const int32_t* n_chars, const int32_t* n_hyps,
                               const int32_t* y_ref, int64_t ref_ld, int64_t ref_cols, int64_t N, int64_t K,
                               int64_t steps, int32_t eos, int64_t L, int32_t* rows, int32_t* hyp_lens, void* stream) {
  if (N < 0 || K < 1 || K > MWER_MAX_M - 1 || steps < 1 || steps > INT32_MAX - 2 || ref_cols < 0 || ref_ld < ref_cols ||
      L < steps + 2 || L < ref_cols || L > INT32_MAX || N * (K + 1) > INT32_MAX)
    return SSASR_EARG;
  if (N == 0) return SSASR_OK;
  if (!chars || !n_chars || !n_hyps || (!y_ref && ref_cols > 0) || !rows || !hyp_lens) return SSASR_EARG;
  hipLaunchKernelGGL(mwer_pack_kernel, dim3((unsigned)(N * (K + 1))), dim3(64), 0, (hipStream_t)stream, chars, n_chars,
                     n_hyps, y_ref, ref_ld, (int)ref_cols, (int)K, (int)steps, (int)eos, (int)L, rows, hyp_lens);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}

extern "C" int ssasr_rows_repeat_fwd(const void* src, int64_t G, int64_t M, int64_t n, void* dst, void* stream) {
  if (!repeat_shape_ok(G, M, n)) return SSASR_EARG;
  if (G == 0) return SSASR_OK;
  if (!src || !dst || ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 3) != 0) return SSASR_EARG;
  hipLaunchKernelGGL(rows_repeat_fwd_kernel, dim3((unsigned)((n + 1023) / 1024), (unsigned)G), dim3(256), 0,
                     (hipStream_t)stream, static_cast<const uint32_t*>(src), (int)M, n, (n & 3) == 0 && aligned16(src, dst),
                     static_cast<uint32_t*>(dst));
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}

extern "C" int ssasr_rows_repeat_bwd(const float* ddst, int64_t G, int64_t M, int64_t n, float* dsrc, void* stream) {
  if (!repeat_shape_ok(G, M, n)) return SSASR_EARG;
  if (G == 0) return SSASR_OK;
  if (!ddst || !dsrc) return SSASR_EARG;
  hipLaunchKernelGGL(rows_repeat_bwd_kernel, dim3((unsigned)((n + 1023) / 1024), (unsigned)G), dim3(256), 0,
                     (hipStream_t)stream, ddst, (int)M, n, (n & 3) == 0 && aligned16(ddst, dsrc), dsrc);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}
