// Attention rescoring of an n-best list (BUILD-DEFINED; include/ssasr.h, "n-best rescoring"): the teacher-forced
// log-probability of every candidate under the Speller's logits (and the CharLM's), the weighted total, the rank and
// the list permuted into rank order, in ONE launch of one workgroup (256 threads) per utterance.
//   1. a wave per (k, t) step of the group's candidates, strided: seq_step_lse / seq_step_term of seq_logp.h, the very
//      device function of the MWER loss; lane 0 leaves the step's term (0 for an unlabelled step) in the term table --
//      LDS when 2 K U doubles fit RESC_LDS_DOUBLES, else the group's slice of the workspace;
//   2. a lane per candidate adds its terms in ascending t and forms the total in double;
//   3. the first wave ranks by counting and writes order / total / parts / lengths;
//   4. all waves copy the texts into rank order.
// Workgroups exchange nothing; no atomics, no spins; every loop is bounded by K, U, V or steps.
#include "seq_logp.h"
#include "../../include/ssasr.h"

namespace {

constexpr int RESC_MAX_K = 32;
constexpr int RESC_MAX_M = 33;
constexpr int RESC_LDS_DOUBLES = 4096;     // 32 KB: the att and lm terms of K U <= 2048 steps

struct RescoreArgs {
  const float* logits;
  const float* lm_logits;
  int64_t lm_row, lm_step;
  const int32_t* y;
  int64_t y_ld;
  const int32_t* n_hyps;
  const float* first;
  const int32_t* chars;
  const int32_t* n_chars;
  double* ws;
  int32_t* order;
  float* total;
  float* parts;
  int32_t* chars_out;
  int32_t* n_chars_out;
  int32_t* n_hyps_out;
  int y_cols, M, K, U, V, steps;
  float att_w, lm_w, first_w, len_w;
};

__global__ __launch_bounds__(256) void rescore_kernel(RescoreArgs a) {
  __shared__ double s_terms[RESC_LDS_DOUBLES];
  __shared__ float s_key[RESC_MAX_K], s_tot[RESC_MAX_K], s_att[RESC_MAX_K], s_lm[RESC_MAX_K];
  __shared__ int s_len[RESC_MAX_K], s_src[RESC_MAX_K];
  const int g = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int K = a.K, U = a.U, V = a.V, M = a.M, steps = a.steps;
  const int n = min(max(a.n_hyps[g], 0), K);
  const int KU = K * U;
  double* att_t = 2 * KU <= RESC_LDS_DOUBLES ? s_terms : a.ws + (int64_t)g * 2 * KU;
  double* lm_t = att_t + KU;

  // 1. the per-step terms of the candidates k < n
  for (int s = wave; s < n * U; s += 4) {
    const int k = s / U, t = s - k * U;
    const int64_t r = (int64_t)g * M + k;
    const int lab = seq_label(a.y + r * a.y_ld, t, a.y_cols, V);     // the same in every lane of the wave
    double ta = 0.0, tl = 0.0;
    if (lab != 0) {
      const float* row = a.logits + (r * U + t) * V;
      ta = seq_step_term(row, lab, seq_step_lse(row, V, lane));
      if (a.lm_logits) {
        const float* lrow = a.lm_logits + r * a.lm_row + (int64_t)t * a.lm_step;
        tl = seq_step_term(lrow, lab, seq_step_lse(lrow, V, lane));
      }
    }
    if (lane == 0) {
      att_t[s] = ta;
      lm_t[s] = tl;
    }
  }
  __syncthreads();

  // 2. a lane per candidate: the sums in ascending t, the total in double, rounded once
  if (tid < n) {
    double att = 0.0, lm = 0.0;
    for (int t = 0; t < U; ++t) {
      att += att_t[tid * U + t];
      lm += lm_t[tid * U + t];
    }
    const int len = min(max(a.n_chars[(int64_t)g * K + tid], 0), steps);
    double tot = 0.0;      // a term whose weight is exactly 0 is left out, not multiplied
    if (a.att_w != 0.f) tot = __dadd_rn(tot, __dmul_rn((double)a.att_w, att));
    if (a.lm_w != 0.f) tot = __dadd_rn(tot, __dmul_rn((double)a.lm_w, lm));
    if (a.first_w != 0.f) tot = __dadd_rn(tot, __dmul_rn((double)a.first_w, (double)a.first[(int64_t)g * K + tid]));
    if (a.len_w != 0.f) tot = __dadd_rn(tot, __dmul_rn((double)a.len_w, (double)len));
    const float tf = (float)tot;
    s_tot[tid] = tf;
    s_key[tid] = tf != tf ? -INFINITY : tf;      // a NaN total ranks as -inf
    s_att[tid] = (float)att;
    s_lm[tid] = (float)lm;
    s_len[tid] = len;
  }
  __syncthreads();

  // 3. rank by counting: the candidates above k, and the equal ones in earlier slots
  if (tid < K) {
    const int64_t o = (int64_t)g * K;
    if (tid < n) {
      const float key = s_key[tid];
      int rank = 0;
      for (int j = 0; j < n; ++j) rank += (s_key[j] > key || (s_key[j] == key && j < tid)) ? 1 : 0;
      s_src[rank] = tid;
      a.order[o + rank] = tid;
      a.total[o + rank] = s_tot[tid];
      a.parts[(o + rank) * 3 + 0] = s_att[tid];
      a.parts[(o + rank) * 3 + 1] = s_lm[tid];
      a.parts[(o + rank) * 3 + 2] = a.first[o + tid];
      a.n_chars_out[o + rank] = s_len[tid];
    } else {                // ranks from n on: an unused slot as ssasr_decode_beam leaves it
      s_src[tid] = -1;
      a.order[o + tid] = -1;
      a.total[o + tid] = 0.f;
      a.parts[(o + tid) * 3 + 0] = 0.f;
      a.parts[(o + tid) * 3 + 1] = 0.f;
      a.parts[(o + tid) * 3 + 2] = 0.f;
      a.n_chars_out[o + tid] = 0;
    }
  }
  if (tid == 0) a.n_hyps_out[g] = n;
  __syncthreads();

  // 4. the texts in rank order, zero from each one's length on
  for (int i = tid; i < K * steps; i += 256) {
    const int rank = i / steps, j = i - rank * steps;
    const int src = s_src[rank];
    int32_t v = 0;
    if (src >= 0 && j < s_len[src]) v = a.chars[((int64_t)g * K + src) * steps + j];
    a.chars_out[(int64_t)g * K * steps + i] = v;
  }
}

bool rescore_shape_ok(int64_t G, int64_t K, int64_t U) {
  return G >= 0 && K >= 1 && K <= RESC_MAX_K && U > 0 && U <= INT32_MAX / (2 * RESC_MAX_K);
}

}  // namespace

extern "C" int64_t ssasr_rescore_ws_bytes(int64_t G, int64_t K, int64_t U) {
  if (!rescore_shape_ok(G, K, U)) return -1;
  return 2 * K * U <= RESC_LDS_DOUBLES ? 0 : G * 2 * K * U * 8;
}

extern "C" int ssasr_rescore(const float* logits, const float* lm_logits, int64_t lm_row_stride,
                             int64_t lm_step_stride, const int32_t* y, int64_t y_ld, int64_t y_cols,
                             const int32_t* n_hyps, const float* first, const int32_t* chars, const int32_t* n_chars,
                             int64_t G, int64_t M, int64_t K, int64_t U, int64_t V, int64_t steps, float att_weight,
                             float lm_weight, float first_weight, float length_bonus, void* ws, int64_t ws_bytes,
                             int32_t* order, float* total, float* parts, int32_t* chars_out, int32_t* n_chars_out,
                             int32_t* n_hyps_out, void* stream) {
  if (!rescore_shape_ok(G, K, U) || M < K || M > RESC_MAX_M || G * M > 65535 || V <= 0 || V > INT32_MAX || steps < 1 ||
      K * steps > INT32_MAX)
    return SSASR_EARG;
  if (!(att_weight - att_weight == 0.f) || !(lm_weight - lm_weight == 0.f) || !(first_weight - first_weight == 0.f) ||
      !(length_bonus - length_bonus == 0.f))
    return SSASR_EARG;                                   // a non-finite weight
  if (G == 0) return SSASR_OK;
  if (y_cols < U + 1 || y_ld < y_cols || y_cols > INT32_MAX) return SSASR_EARG;
  if (lm_logits && (lm_row_stride < V || lm_step_stride < V)) return SSASR_EARG;
  const int64_t need = ssasr_rescore_ws_bytes(G, K, U);
  if (need > 0 && (!ws || (reinterpret_cast<uintptr_t>(ws) & 7) != 0 || ws_bytes < need)) return SSASR_EARG;
  if (!logits || !y || !n_hyps || !first || !chars || !n_chars || !order || !total || !parts || !chars_out ||
      !n_chars_out || !n_hyps_out)
    return SSASR_EARG;
  RescoreArgs a;
  a.logits = logits; a.lm_logits = lm_logits; a.lm_row = lm_row_stride; a.lm_step = lm_step_stride;
  a.y = y; a.y_ld = y_ld; a.n_hyps = n_hyps; a.first = first; a.chars = chars; a.n_chars = n_chars;
  a.ws = static_cast<double*>(ws);
  a.order = order; a.total = total; a.parts = parts; a.chars_out = chars_out; a.n_chars_out = n_chars_out;
  a.n_hyps_out = n_hyps_out;
  a.y_cols = (int)y_cols; a.M = (int)M; a.K = (int)K; a.U = (int)U; a.V = (int)V; a.steps = (int)steps;
  a.att_w = att_weight; a.lm_w = lm_weight; a.first_w = first_weight; a.len_w = length_bonus;
  hipLaunchKernelGGL(rescore_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, a);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}
