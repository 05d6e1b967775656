// Inference: the greedy decode loop of ASR.decode (src/asr.py:112-173) with the CharLM term
// (src/charlm.py:46-57) as ONE launch for N encoded utterances, the same loop as a beam search over up to 32
// hypotheses per utterance (decode_beam_kernel, below) and as up to 32 samples per utterance drawn from the model's
// own distribution (decode_sample_kernel), and one CharLM step for callers that drive the language model themselves.
//
// One workgroup owns one utterance for its whole loop.  Nothing is exchanged between workgroups:
// no status words, no spins, no arena.  Every loop is bounded by max_steps / enc_len / a dimension,
// and a workgroup whose utterance emitted <EOS> zeroes the rest of its output rows and exits.
// Decoder and LM states stay in LDS for the whole loop; weights, feat and comp are streamed from
// L2 / HBM every step as whole rows, 16 bytes per lane (feat at T' = 375 does not fit LDS).
// A matrix-vector product gives each wave four rows at a time; a row's partial sums are reduced
// on the DPP network (common.h, wave_sum).  What a workgroup computes for its utterance depends
// on that utterance's frames and enc_len alone, never on N or the padded T': an utterance decoded
// in a batch gives the bits it gives alone.
//
// The four kernels are built from one set of step helpers, each over n hypotheses whose rows lie a stride apart
// (the greedy kernel and the CharLM step pass n = 1): matmat_n / matvec / matmat (weight rows x input vectors, comp =
// tanh(psi(feat)) included), lstm_update, gru_update, context_partial + context_reduce (att . feat) and score_row
// (log_softmax(asr) + lm_weight * log_softmax(lm)).  The two K-hypothesis kernels also share the SEQUENCE that calls
// them: decode_prologue (comp, zero states, <SOS>) and speller_step (phases 1 to 7, barriers included) over a StepWs;
// what follows the score rows is theirs (the beam's selection, back-pointers and output / the sampler's draw).
// decode_greedy_kernel and charlm_step_kernel keep bodies of their own: state in LDS behind __syncthreads() alone, a
// block-wide softmax over the frames (another summation order than a wave per hypothesis) and a comp prologue shaped
// to stay out of scratch memory.
#include <cmath>
#include "../../include/ssasr.h"
#include "common.h"
#include "ctc_prefix.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kRows = 4;                 // rows of a matrix-vector product a wave has in flight
constexpr int kHyps = 8;                 // input vectors one pass of matmat holds against a weight row group
constexpr size_t kMaxLds = 160 * 1024;   // LDS of one CU

__device__ __forceinline__ float dot4(const float4& a, const float4& b, float acc) {
  acc = fmaf(a.x, b.x, acc);
  acc = fmaf(a.y, b.y, acc);
  acc = fmaf(a.z, b.z, acc);
  return fmaf(a.w, b.w, acc);
}
__device__ __forceinline__ float sigmoid_exact(float x) { return 1.0f / (1.0f + expf(-x)); }

// out[b * os + r] = act(w1[r][0..k1) . x1[b * xs1 ..] + w2[r][0..k2) . x2[b * xs2 ..] + b1[r] + b2[r]) for r < rows,
// b < nb <= NB; rows and vectors 16-byte aligned, k1 / k2 multiples of 4 (k2 = 0: one segment); b1 / b2 optional;
// act 1 = tanh.  Called by every wave of the workgroup; rows are dealt to waves in groups of kRows.
template <int NB>
__device__ void matmat_n(const float* w1, int64_t ld1, const float* x1, int64_t xs1, int k1,
                         const float* w2, int64_t ld2, const float* x2, int64_t xs2, int k2,
                         const float* __restrict__ b1, const float* __restrict__ b2, int rows, int act,
                         float* out, int64_t os, int nb) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r0 = wave * kRows; r0 < rows; r0 += kWaves * kRows) {
    float acc[kRows][NB];
    const float* p1[kRows];
    const float* p2[kRows];
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      const int r = min(r0 + j, rows - 1);          // rows past the end repeat the last one and are dropped
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[j][b] = 0.f;
      p1[j] = w1 + (int64_t)r * ld1;
      p2[j] = k2 ? w2 + (int64_t)r * ld2 : nullptr;
    }
    for (int k = lane * 4; k < k1; k += 256) {
      float4 w[kRows];
#pragma unroll
      for (int j = 0; j < kRows; ++j) w[j] = *reinterpret_cast<const float4*>(p1[j] + k);
#pragma unroll
      for (int b = 0; b < NB; ++b) {                // vectors past nb repeat the last one and are dropped
        const float4 x = *reinterpret_cast<const float4*>(x1 + (int64_t)min(b, nb - 1) * xs1 + k);
#pragma unroll
        for (int j = 0; j < kRows; ++j) acc[j][b] = dot4(w[j], x, acc[j][b]);
      }
    }
    for (int k = lane * 4; k < k2; k += 256) {
      float4 w[kRows];
#pragma unroll
      for (int j = 0; j < kRows; ++j) w[j] = *reinterpret_cast<const float4*>(p2[j] + k);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const float4 x = *reinterpret_cast<const float4*>(x2 + (int64_t)min(b, nb - 1) * xs2 + k);
#pragma unroll
        for (int j = 0; j < kRows; ++j) acc[j][b] = dot4(w[j], x, acc[j][b]);
      }
    }
    float v = 0.f;                                  // lane j * NB + b keeps the sum of row j, vector b
#pragma unroll
    for (int j = 0; j < kRows; ++j)
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const float s = wave_sum(acc[j][b]);
        if (lane == j * NB + b) v = s;
      }
    const int j = lane / NB, b = lane % NB;
    if (lane < kRows * NB && r0 + j < rows && b < nb) {
      const int r = r0 + j;
      if (b1) v += b1[r];
      if (b2) v += b2[r];
      out[(int64_t)b * os + r] = act == 1 ? tanhf(v) : v;
    }
  }
}

// matmat_n over n vectors, kHyps at a time; the last pass takes the narrowest form that holds what is left
__device__ void matmat(const float* w1, int64_t ld1, const float* x1, int64_t xs1, int k1,
                       const float* w2, int64_t ld2, const float* x2, int64_t xs2, int k2,
                       const float* __restrict__ b1, const float* __restrict__ b2, int rows, int act,
                       float* out, int64_t os, int n) {
  for (int b0 = 0; b0 < n; b0 += kHyps) {
    const int nb = min(kHyps, n - b0);
    const float* y1 = x1 + (int64_t)b0 * xs1;
    const float* y2 = k2 ? x2 + (int64_t)b0 * xs2 : nullptr;
    float* o = out + (int64_t)b0 * os;
    if (nb == 1) matmat_n<1>(w1, ld1, y1, xs1, k1, w2, ld2, y2, xs2, k2, b1, b2, rows, act, o, os, nb);
    else if (nb == 2) matmat_n<2>(w1, ld1, y1, xs1, k1, w2, ld2, y2, xs2, k2, b1, b2, rows, act, o, os, nb);
    else if (nb <= 4) matmat_n<4>(w1, ld1, y1, xs1, k1, w2, ld2, y2, xs2, k2, b1, b2, rows, act, o, os, nb);
    else matmat_n<kHyps>(w1, ld1, y1, xs1, k1, w2, ld2, y2, xs2, k2, b1, b2, rows, act, o, os, nb);
  }
}

// one vector: the matrix-vector products of decode_greedy_kernel and charlm_step_kernel
__device__ void matvec(const float* w1, int64_t ld1, const float* x1, int k1,
                       const float* w2, int64_t ld2, const float* x2, int k2,
                       const float* __restrict__ b1, const float* __restrict__ b2, int rows, int act, float* out) {
  matmat_n<1>(w1, ld1, x1, 0, k1, w2, ld2, x2, 0, k2, b1, b2, rows, act, out, 0, 1);
}

// nn.LSTMCell's update of n hypotheses from their pre-activations [4H] (order i, f, g, o; src/asr.py:320-324);
// gs / ss: floats from one hypothesis' gate row / state rows to the next one's
__device__ void lstm_update(const float* gates, int64_t gs, float* h0, float* c0, int64_t ss, int H, int n) {
  for (int e = threadIdx.x; e < n * H; e += kThreads) {
    const int b = e / H, u = e % H;
    const float* g = gates + b * gs;
    float *h = h0 + b * ss, *c = c0 + b * ss;
    const float i = sigmoid_exact(g[u]), f = sigmoid_exact(g[H + u]), gg = tanhf(g[2 * H + u]),
                o = sigmoid_exact(g[3 * H + u]);
    const float cn = f * c[u] + i * gg;
    c[u] = cn;
    h[u] = o * tanhf(cn);
  }
}

// nn.GRUCell's update of n hypotheses from gi = W_ih x + b_ih and gh = W_hh h + b_hh [3H] (order r, z, n);
// gs / hs: floats from one hypothesis' gi and gh rows / state row to the next one's
__device__ void gru_update(const float* gi0, const float* gh0, int64_t gs, float* h0, int64_t hs, int H, int n) {
  for (int e = threadIdx.x; e < n * H; e += kThreads) {
    const int b = e / H, u = e % H;
    const float *gi = gi0 + b * gs, *gh = gh0 + b * gs;
    float* h = h0 + b * hs;
    const float r = sigmoid_exact(gi[u] + gh[u]), z = sigmoid_exact(gi[H + u] + gh[H + u]);
    const float n = tanhf(gi[2 * H + u] + r * gh[2 * H + u]);
    h[u] = (1.f - z) * n + z * h[u];
  }
}

// frame groups of the context sum: kThreads threads over the E / 4 float4 columns
__host__ __device__ inline int context_groups(int E) { return E / 4 >= kThreads ? 1 : kThreads / (E / 4); }

// context = att . feat (src/asr.py:389-390) of n hypotheses whose attention rows lie `as` floats apart: a thread
// sums one float4 column over the frames g, g + G, ... of its group for NH hypotheses at a time, so feat is read
// once per NH of them.  Group g's sums of hypothesis b go to dst + g * gs + b * ds: with G == 1 that is the context
// itself, otherwise the partial sums that context_reduce adds up.
template <int NH>
__device__ void context_partial(const float* feat, int E, int len, int G, const float* att0, int64_t as, int n,
                                float* dst, int64_t gs, int64_t ds) {
  const int tid = threadIdx.x, ncol4 = E / 4;
  for (int b0 = 0; b0 < n; b0 += NH) {
    const int nb = min(NH, n - b0);
    const float* att = att0 + b0 * as;
    const int g = G == 1 ? 0 : tid / ncol4;
    for (int c = G == 1 ? tid : tid % ncol4; c < ncol4 && g < G; c += kThreads) {
      float4 s[NH];
#pragma unroll
      for (int j = 0; j < NH; ++j) s[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int t = g; t < len; t += G) {
        const float4 v = *reinterpret_cast<const float4*>(feat + (int64_t)t * E + c * 4);
#pragma unroll
        for (int j = 0; j < NH; ++j)
          if (j < nb) {
            const float a = att[j * as + t];
            s[j].x = fmaf(a, v.x, s[j].x); s[j].y = fmaf(a, v.y, s[j].y);
            s[j].z = fmaf(a, v.z, s[j].z); s[j].w = fmaf(a, v.w, s[j].w);
          }
      }
#pragma unroll
      for (int j = 0; j < NH; ++j)
        if (j < nb) *reinterpret_cast<float4*>(dst + g * gs + (b0 + j) * ds + c * 4) = s[j];
    }
  }
}

// ctx[b * cs + e] = part[b * ps + e] + part[gs + b * ps + e] + ... over the G groups, in that order; b < n, e < E
__device__ void context_reduce(const float* part, int64_t gs, int64_t ps, int G, float* ctx, int64_t cs, int E, int n) {
  for (int i = threadIdx.x; i < n * E; i += kThreads) {
    const int b = i / E, e = i % E;
    float s = part[b * ps + e];
    for (int g = 1; g < G; ++g) s += part[g * gs + b * ps + e];
    ctx[b * cs + e] = s;
  }
}

// This lane's log_softmax(asr)[lane] + lm_weight * log_softmax(lm)[lane] (src/asr.py:153-157) from the logit rows
// lg and lmlg (nullptr: no language model).  Called by a whole wave (V <= 64); what a lane >= V gets is no score.
__device__ float score_row(const float* lg, const float* lmlg, int V, float lm_weight) {
  const int lane = threadIdx.x & 63;
  const float x = lane < V ? lg[lane] : -INFINITY;
  const float xm = wave_max(x);
  const float xs = wave_sum(lane < V ? expf(x - xm) : 0.f);
  float fin = x - xm - logf(xs);
  if (lmlg) {
    const float y = lane < V ? lmlg[lane] : -INFINITY;
    const float ym = wave_max(y);
    const float ys = wave_sum(lane < V ? expf(y - ym) : 0.f);
    fin = fin + lm_weight * (y - ym - logf(ys));
  }
  return fin;
}

__device__ void copy_row(float* dst, const float* __restrict__ src, int n) {
  for (int i = threadIdx.x; i < n; i += kThreads) dst[i] = src[i];
}

struct LmDev {
  int H;                         // 0: no language model
  const float *emb, *w_ih1, *w_hh1, *b_ih1, *b_hh1, *w_ih2, *w_hh2, *b_ih2, *b_hh2, *w_out, *b_out;
};

struct InferDev {
  int T, E, A, D, V, max_steps, eos;
  float lm_weight;
  const float* feat;
  const int32_t* enc_len;
  float* comp;
  const float *w_psi, *b_psi, *w_phi;
  const float *w_ih1, *w_hh1, *b_ih1, *b_hh1, *w_ih2, *w_hh2, *b_ih2, *b_hh2;
  const float *embed, *w_ct, *b_ct;
  LmDev lm;
  int32_t* chars;
  int32_t* n_chars;
  float* scores;
  float* att;
};

__host__ __device__ inline int up4(int v) { return (v + 3) & ~3; }

// LDS map (floats); every block starts on 16 bytes
struct Lds {
  int h1, c1, h2, c2, xin, q, gates, e, part, red, lg, lmlg, lmx, lmh1, lmh2, gi, gh, total;
};
__host__ __device__ inline Lds lds_map(int T, int E, int A, int D, int Hl) {
  Lds m;
  int o = 0;
  m.h1 = o; o += D;
  m.c1 = o; o += D;
  m.h2 = o; o += D;
  m.c2 = o; o += D;
  m.xin = o; o += D + E;            // [embedding of the last character | context], src/asr.py:149
  m.q = o; o += A;
  m.gates = o; o += 4 * D;
  m.e = o; o += up4(T);             // energies, then attention weights
  m.part = o; o += kThreads * 4;    // partial context sums
  m.red = o; o += 32;               // per-wave partials of the block reductions, the winner
  m.lg = o; o += 64;
  m.lmlg = o; o += 64;
  m.lmx = o; o += Hl;
  m.lmh1 = o; o += Hl;
  m.lmh2 = o; o += Hl;
  m.gi = o; o += 3 * Hl;
  m.gh = o; o += 3 * Hl;
  m.total = o;
  return m;
}

__device__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float m = red[0];
  for (int w = 1; w < kWaves; ++w) m = fmaxf(m, red[w]);
  return m;
}
__device__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
  for (int w = 1; w < kWaves; ++w) s += red[w];
  return s;
}

__global__ __launch_bounds__(kThreads) void decode_greedy_kernel(InferDev p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = p.T, E = p.E, A = p.A, D = p.D, V = p.V, Hl = p.lm.H;
  const Lds m = lds_map(T, E, A, D, Hl);
  float *h1 = lds + m.h1, *c1 = lds + m.c1, *h2 = lds + m.h2, *c2 = lds + m.c2, *xin = lds + m.xin, *q = lds + m.q,
        *gates = lds + m.gates, *en = lds + m.e, *part = lds + m.part, *red = lds + m.red, *lg = lds + m.lg,
        *lmlg = lds + m.lmlg, *lmx = lds + m.lmx, *lmh1 = lds + m.lmh1, *lmh2 = lds + m.lmh2, *gi = lds + m.gi,
        *gh = lds + m.gh;
  int* winner = reinterpret_cast<int*>(red + 16);

  const int len = min(max(p.enc_len[n], 1), T);      // frames this utterance attends over
  const float* feat = p.feat + (int64_t)n * T * E;
  float* comp = p.comp + (int64_t)n * T * A;
  int32_t* chars = p.chars + (int64_t)n * p.max_steps;
  float* scores = p.scores + (int64_t)n * p.max_steps * V;
  float* att = p.att ? p.att + (int64_t)n * p.max_steps * T : nullptr;

  // comp = tanh(psi(feat)) for this utterance's frames, once (src/asr.py:381): W_psi against the frames as vectors,
  // kRows of them a pass (matmat's kHyps accumulator sets would cost this kernel scratch memory)
  for (int t0 = 0; t0 < len; t0 += kRows)
    matmat_n<kRows>(p.w_psi, E, feat + (int64_t)t0 * E, E, E, nullptr, 0, nullptr, 0, 0, p.b_psi, nullptr, A, 1,
                    comp + (int64_t)t0 * A, A, min(kRows, len - t0));
  // zero states (src/asr.py:133-134), <SOS> = 0 as the first input character (:137-138)
  for (int i = tid; i < 4 * D; i += kThreads) lds[m.h1 + i] = 0.f;
  for (int i = tid; i < 2 * Hl; i += kThreads) lmh1[i] = 0.f;       // lmh1 and lmh2 are adjacent
  copy_row(xin, p.embed, D);
  if (Hl) copy_row(lmx, p.lm.emb, Hl);
  __syncthreads();

  const int G = context_groups(E);
  int step = 0, emitted = p.max_steps;
  for (; step < p.max_steps; ++step) {
    // 1: q = tanh(phi(h1)) (src/asr.py:383) | LM layer 1 products (src/charlm.py:54)
    matvec(p.w_phi, D, h1, D, nullptr, 0, nullptr, 0, nullptr, nullptr, A, 1, q);
    if (Hl) {
      matvec(p.lm.w_ih1, Hl, lmx, Hl, nullptr, 0, nullptr, 0, p.lm.b_ih1, nullptr, 3 * Hl, 0, gi);
      matvec(p.lm.w_hh1, Hl, lmh1, Hl, nullptr, 0, nullptr, 0, p.lm.b_hh1, nullptr, 3 * Hl, 0, gh);
    }
    __syncthreads();
    // 2: energies over the utterance's frames (src/asr.py:385-387) | LM layer 1 update
    if (Hl) gru_update(gi, gh, 0, lmh1, 0, Hl, 1);
    matvec(comp, A, q, A, nullptr, 0, nullptr, 0, nullptr, nullptr, len, 0, en);
    __syncthreads();
    // 3: softmax over the frames (src/asr.py:388) | LM layer 2 products (src/charlm.py:55).  Block-wide here, a wave
    // per hypothesis in decode_beam_kernel: the two sum in different orders, so one form for both would change the
    // bits and the time of one of them
    float mx = -INFINITY;
    for (int t = tid; t < len; t += kThreads) mx = fmaxf(mx, en[t]);
    mx = block_max(mx, red);
    float sum = 0.f;
    for (int t = tid; t < len; t += kThreads) {
      const float ex = expf(en[t] - mx);
      en[t] = ex;
      sum += ex;
    }
    sum = block_sum(sum, red);
    for (int t = tid; t < len; t += kThreads) en[t] = en[t] / sum;
    if (att) {
      float* row = att + (int64_t)step * T;
      for (int t = tid; t < T; t += kThreads) row[t] = t < len ? en[t] : 0.f;
    }
    if (Hl) {
      matvec(p.lm.w_ih2, Hl, lmh1, Hl, nullptr, 0, nullptr, 0, p.lm.b_ih2, nullptr, 3 * Hl, 0, gi);
      matvec(p.lm.w_hh2, Hl, lmh2, Hl, nullptr, 0, nullptr, 0, p.lm.b_hh2, nullptr, 3 * Hl, 0, gh);
    }
    __syncthreads();
    // 4: context = att . feat (src/asr.py:389-390), partial sums in LDS at [g][E] | LM layer 2 update
    context_partial<1>(feat, E, len, G, en, 0, 1, G == 1 ? xin + D : part, E, 0);
    if (Hl) gru_update(gi, gh, 0, lmh2, 0, Hl, 1);
    __syncthreads();
    if (G > 1) {
      context_reduce(part, E, 0, G, xin + D, 0, E, 1);
      __syncthreads();
    }
    // 5: Speller cell 1 on [embedding | context] (src/asr.py:149-150, :320-321) | LM output layer (src/charlm.py:56)
    matvec(p.w_ih1, D + E, xin, D + E, p.w_hh1, D, h1, D, p.b_ih1, p.b_hh1, 4 * D, 0, gates);
    if (Hl) matvec(p.lm.w_out, Hl, lmh2, Hl, nullptr, 0, nullptr, 0, p.lm.b_out, nullptr, V, 0, lmlg);
    __syncthreads();
    lstm_update(gates, 0, h1, c1, 0, D, 1);
    __syncthreads();
    // 6: cell 2 (src/asr.py:323-324)
    matvec(p.w_ih2, D, h1, D, p.w_hh2, D, h2, D, p.b_ih2, p.b_hh2, 4 * D, 0, gates);
    __syncthreads();
    lstm_update(gates, 0, h2, c2, 0, D, 1);
    __syncthreads();
    // 7: char_trans (src/asr.py:153)
    matvec(p.w_ct, D, h2, D, nullptr, 0, nullptr, 0, p.b_ct, nullptr, V, 0, lg);
    __syncthreads();
    // 8: final = log_softmax(asr) + lm_weight * log_softmax(lm), first maximum wins (src/asr.py:153-159)
    if (wave == 0) {
      float fin = score_row(lg, Hl ? lmlg : nullptr, V, p.lm_weight);
      if (lane >= V) fin = -INFINITY;
      const float best = wave_max(fin);
      unsigned long long hit = __ballot(lane < V && fin == best);
      if (hit == 0) hit = __ballot(lane < V && fin != fin);       // a NaN row: torch.argmax takes the first NaN
      const int w = hit ? __ffsll(hit) - 1 : 0;
      if (lane < V) scores[(int64_t)step * V + lane] = fin;
      if (lane == 0) {
        chars[step] = w;
        *winner = w;
      }
    }
    __syncthreads();
    const int w = *winner;
    if (w == p.eos) {              // src/asr.py:167-169: <EOS> ends the loop and is not part of the text
      emitted = step;
      ++step;
      break;
    }
    copy_row(xin, p.embed + (int64_t)w * D, D);                    // src/asr.py:161-162
    if (Hl) copy_row(lmx, p.lm.emb + (int64_t)w * Hl, Hl);
    __syncthreads();
  }
  // `step` rows were written; the rest of this utterance's outputs are zero
  if (tid == 0) p.n_chars[n] = emitted;
  for (int64_t i = (int64_t)step + tid; i < p.max_steps; i += kThreads) chars[i] = 0;
  for (int64_t i = (int64_t)step * V + tid; i < (int64_t)p.max_steps * V; i += kThreads) scores[i] = 0.f;
  if (att)
    for (int64_t i = (int64_t)step * T + tid; i < (int64_t)p.max_steps * T; i += kThreads) att[i] = 0.f;
}

// ---- beam search ------------------------------------------------------------------------------------------------
// decode_beam_kernel: the loop above for up to K hypotheses of one utterance in ONE workgroup.
// Layout.  A workgroup owns an utterance for the whole loop, as in decode_greedy_kernel; nothing is exchanged
// between workgroups, nothing spins, and every loop is bounded by max_steps, enc_len, K or a dimension.
// comp = tanh(psi(feat)) is computed once and shared by all hypotheses.  Every weight matrix is streamed ONCE
// per step for all live hypotheses: matmat keeps kRows weight rows against up to kHyps input vectors in flight
// (kRows * kHyps accumulators per lane); more than kHyps live hypotheses take one pass per kHyps.  feat is
// streamed once per step for the context sums of all live hypotheses in the same way.
// Where the state lives (one rule, whatever the sizes): everything that is per hypothesis -- h1, c1, h2, c2 and
// the LM's two hidden rows (double-buffered: after the selection a new slot's state is a COPY of its parent's
// row into the other buffer, never an in-place shuffle), the step's inputs and intermediates (embedding |
// context, q, gates, energies, LM gates, logits) and the back-pointers (parent, char) per step and slot -- is
// in the caller's workspace in global memory, a slice per workgroup that no other workgroup touches (about
// 8 KB of state per hypothesis at D 256, E 512, Hl 128: 32 hypotheses do not fit 160 KB of LDS).  The slice is
// L2 / L1 resident; writer and reader phases are separated by phase_sync(): a workgroup-scope fence and the
// workgroup barrier.  LDS holds only what the selection needs: the K * 64 candidate scores, the hypotheses'
// scores, the chosen / finished lists and the reduction scratch (about 10 KB, static).
// Selection: at most K * V <= 32 * 64 candidates score_b + row_b[v]; W = min(K - finished, live * V) rounds of a
// block-wide arg-max, ties to the lower flat index b * 64 + v (the order of b * V + v); a chosen candidate is
// struck out with a NaN, which no score can be (NaN rows are scored -inf).
// An utterance's results depend on its frames, enc_len, K and max_steps alone, never on N or the padded T.
constexpr int kMaxBeam = 32;
constexpr int kNone = 1 << 30;

__device__ __forceinline__ void phase_sync() {
  __threadfence_block();
  __syncthreads();
}

// workspace slice of one utterance (floats; every block starts on 16 bytes)
struct BeamWs {
  int64_t st, xin, lmx, q, gates, en, part, gi, gh, lg, lmlg, bp, total;
  int Sz, Tp, G;
};
__host__ __device__ inline int64_t up4l(int64_t v) { return (v + 3) & ~(int64_t)3; }
// bufs: copies of the K state rows (the beam search re-parents from one buffer into the other, the sampler keeps one);
// bp: int32 back-pointer words (the sampler writes its characters straight to the output)
__host__ __device__ inline BeamWs decode_ws_map(int K, int T, int E, int A, int D, int Hl, int bufs, int64_t bp) {
  BeamWs m;
  m.Sz = 4 * D + 2 * Hl;                  // h1 | c1 | h2 | c2 | LM h1 | LM h2 of one hypothesis
  m.Tp = up4(T);
  m.G = context_groups(E);
  int64_t o = 0;
  m.st = o; o += bufs * (int64_t)K * m.Sz;
  m.xin = o; o += (int64_t)K * (D + E);   // [embedding of the last character | context]
  m.lmx = o; o += (int64_t)K * Hl;
  m.q = o; o += (int64_t)K * A;
  m.gates = o; o += (int64_t)K * 4 * D;
  m.en = o; o += (int64_t)K * m.Tp;       // energies, then attention weights
  m.part = o; o += m.G > 1 ? (int64_t)m.G * K * E : 0;   // partial context sums [G][K][E]
  m.gi = o; o += (int64_t)K * 3 * Hl;
  m.gh = o; o += (int64_t)K * 3 * Hl;
  m.lg = o; o += (int64_t)K * 64;
  m.lmlg = o; o += (int64_t)K * 64;
  m.bp = o; o += up4l(bp);
  m.total = up4l(o);
  return m;
}
// two buffers of K rows; int32 back-pointers [S][K]: parent | char << 8
__host__ __device__ inline BeamWs beam_ws_map(int K, int T, int E, int A, int D, int Hl, int S) {
  return decode_ws_map(K, T, E, A, D, Hl, 2, (int64_t)S * K);
}
__host__ __device__ inline BeamWs sample_ws_map(int K, int T, int E, int A, int D, int Hl) {
  return decode_ws_map(K, T, E, A, D, Hl, 1, 0);
}

// A wave's half of the softmax over one hypothesis' frames: row[t] = exp(row[t] - max) for t < len; returns the
// sum, in every lane.  The caller divides (the coverage form of the beam search folds its counts into that pass).
__device__ __forceinline__ float wave_exp_row(float* row, int len) {
  const int lane = threadIdx.x & 63;
  float mx = -INFINITY;
  for (int t = lane; t < len; t += 64) mx = fmaxf(mx, row[t]);
  mx = wave_max(mx);
  float sum = 0.f;
  for (int t = lane; t < len; t += 64) {
    const float ex = expf(row[t] - mx);
    row[t] = ex;
    sum += ex;
  }
  return wave_sum(sum);
}
__device__ __forceinline__ void normalise_row(float* row, float sum, int len) {
  for (int t = (threadIdx.x & 63); t < len; t += 64) row[t] = row[t] / sum;
}

// one utterance's blocks of a BeamWs slice that a step reads and writes, K slots each, and the strides between slots
struct StepWs {
  float *xin, *lmx, *q, *gates, *en, *part, *gi, *gh, *lg, *lmlg;
  int K, Sz, Tp, G, XI;
};
__device__ __forceinline__ StepWs step_ws(const BeamWs& m, float* ws, int K, int XI) {
  return StepWs{ws + m.xin, ws + m.lmx, ws + m.q, ws + m.gates, ws + m.en, ws + m.part, ws + m.gi, ws + m.gh,
                ws + m.lg, ws + m.lmlg, K, m.Sz, m.Tp, m.G, XI};
}

// Before the loop: comp = tanh(psi(feat)) for this utterance's frames, once, shared by every slot (W_psi against the
// frames as vectors); slots 0 .. n - 1 of st: zero states, <SOS> = 0 as the input character.  No barrier.
__device__ __forceinline__ void decode_prologue(const InferDev& p, const StepWs& w, const float* feat, float* comp,
                                                int len, float* st, int n) {
  const int tid = threadIdx.x, D = p.D, Hl = p.lm.H;
  matmat(p.w_psi, p.E, feat, p.E, p.E, nullptr, 0, nullptr, 0, 0, p.b_psi, nullptr, p.A, 1, comp, p.A, len);
  for (int i = tid; i < n * w.Sz; i += kThreads) st[i] = 0.f;
  for (int i = tid; i < n * D; i += kThreads) w.xin[(int64_t)(i / D) * w.XI + i % D] = p.embed[i % D];
  for (int i = tid; i < n * Hl; i += kThreads) w.lmx[i] = p.lm.emb[i % Hl];
}

// Phases 1 to 7 of one step for slots 0 .. n - 1 of the state rows st (w.Sz floats apart), up to and including the
// phase_sync() after char_trans: w.lg / w.lmlg hold the slots' logit rows.  att_row(b, row, sum) is called by the wave
// that owns slot b once row holds exp(energy - max) and sum their sum: it leaves the attention weights in row
// (normalise_row; the beam search's coverage form counts in the same pass).
template <class AttRow>
__device__ __forceinline__ void speller_step(const InferDev& p, const StepWs& w, const float* feat, const float* comp,
                                             int len, float* st, int n, AttRow att_row) {
  const int wave = threadIdx.x >> 6;
  const int E = p.E, A = p.A, D = p.D, V = p.V, Hl = p.lm.H, K = w.K, Sz = w.Sz, Tp = w.Tp, G = w.G, XI = w.XI;
  float *h1 = st, *c1 = st + D, *h2 = st + 2 * D, *c2 = st + 3 * D, *lmh1 = st + 4 * D, *lmh2 = lmh1 + Hl;
  float *xin = w.xin, *lmx = w.lmx, *q = w.q, *gates = w.gates, *en = w.en, *part = w.part, *gi = w.gi, *gh = w.gh;
  // 1: q = tanh(phi(h1)) | LM layer 1 products
  matmat(p.w_phi, D, h1, Sz, D, nullptr, 0, nullptr, 0, 0, nullptr, nullptr, A, 1, q, A, n);
  if (Hl) {
    matmat(p.lm.w_ih1, Hl, lmx, Hl, Hl, nullptr, 0, nullptr, 0, 0, p.lm.b_ih1, nullptr, 3 * Hl, 0, gi, 3 * Hl, n);
    matmat(p.lm.w_hh1, Hl, lmh1, Sz, Hl, nullptr, 0, nullptr, 0, 0, p.lm.b_hh1, nullptr, 3 * Hl, 0, gh, 3 * Hl, n);
  }
  phase_sync();
  // 2: energies over the utterance's frames | LM layer 1 update
  gru_update(gi, gh, 3 * Hl, lmh1, Sz, Hl, n);
  matmat(comp, A, q, A, A, nullptr, 0, nullptr, 0, 0, nullptr, nullptr, len, 0, en, Tp, n);
  phase_sync();
  // 3: softmax over the frames, a wave per slot (decode_greedy_kernel's is block-wide) | LM layer 2 products
  for (int b = wave; b < n; b += kWaves) {
    float* row = en + (int64_t)b * Tp;
    const float sum = wave_exp_row(row, len);
    att_row(b, row, sum);
  }
  if (Hl) {
    matmat(p.lm.w_ih2, Hl, lmh1, Sz, Hl, nullptr, 0, nullptr, 0, 0, p.lm.b_ih2, nullptr, 3 * Hl, 0, gi, 3 * Hl, n);
    matmat(p.lm.w_hh2, Hl, lmh2, Sz, Hl, nullptr, 0, nullptr, 0, 0, p.lm.b_hh2, nullptr, 3 * Hl, 0, gh, 3 * Hl, n);
  }
  phase_sync();
  // 4: context = att . feat, partial sums in the workspace at [g][K][E] | LM layer 2 update
  context_partial<kHyps>(feat, E, len, G, en, Tp, n, G == 1 ? xin + D : part, (int64_t)K * E, G == 1 ? XI : E);
  gru_update(gi, gh, 3 * Hl, lmh2, Sz, Hl, n);
  phase_sync();
  if (G > 1) {
    context_reduce(part, (int64_t)K * E, E, G, xin + D, XI, E, n);
    phase_sync();
  }
  // 5: Speller cell 1 on [embedding | context] | LM output layer
  matmat(p.w_ih1, XI, xin, XI, XI, p.w_hh1, D, h1, Sz, D, p.b_ih1, p.b_hh1, 4 * D, 0, gates, 4 * D, n);
  if (Hl) matmat(p.lm.w_out, Hl, lmh2, Sz, Hl, nullptr, 0, nullptr, 0, 0, p.lm.b_out, nullptr, V, 0, w.lmlg, 64, n);
  phase_sync();
  lstm_update(gates, 4 * D, h1, c1, Sz, D, n);
  phase_sync();
  // 6: cell 2
  matmat(p.w_ih2, D, h1, Sz, D, p.w_hh2, D, h2, Sz, D, p.b_ih2, p.b_hh2, 4 * D, 0, gates, 4 * D, n);
  phase_sync();
  lstm_update(gates, 4 * D, h2, c2, Sz, D, n);
  phase_sync();
  // 7: char_trans
  matmat(p.w_ct, D, h2, Sz, D, nullptr, 0, nullptr, 0, 0, p.b_ct, nullptr, V, 0, w.lg, 64, n);
  phase_sync();
}

struct BeamDev {
  InferDev in;                            // in.chars [N][K][S], in.n_chars [N][K]; in.scores / in.att unused
  int K;
  float* ws;
  float* hyp_scores;
  int32_t* n_hyps;
};

// ---- CTC prefix scores (joint CTC / attention decoding; semantics in include/ssasr.h) -----------------------------
// The CTC form of decode_beam_kernel adds, per utterance: lp = log_softmax(W_ctc feat_t + b_ctc) [len][64] (once,
// before the loop, like comp), per live hypothesis g the two lattice rows gamma_n^g, gamma_b^g [T] (double-buffered
// like the Speller state: a new slot's rows are written into the other buffer from its parent's) and psi(g).  All of
// it is in the workspace slice behind what the plain form uses (T goes to 16,384: nothing of it may be assumed to fit
// LDS); only the step's per-candidate psi (K * 64 doubles) and the hypotheses' last characters are in LDS.
// gamma and psi are doubles; every exp / log runs in float on a DIFFERENCE from the larger operand / the running
// maximum (ctc.hip's rule, DESIGN 4.7: a float lattice of magnitude ~ nll loses 2e-4 relative).
struct CtcDev {
  const float *w, *b;                     // ctc_head [V][E], [V]
  float lambda;
  int blank;
};

// what the CTC form adds behind BeamWs' blocks (offsets in floats, from the slice's start; the doubles start on
// 16 bytes); total: the CTC form's slice
struct CtcWs {
  int64_t lp, gam, psi, total;
};
__host__ __device__ inline CtcWs ctc_ws_map(const BeamWs& m, int K, int T) {
  CtcWs c;
  int64_t o = m.total;
  c.lp = o; o += (int64_t)T * 64;               // float [T][64]
  c.gam = o; o += 2 * (2 * (int64_t)K * 2 * T); // double [2 buffers][K][gamma_n | gamma_b][T]
  c.psi = o; o += 2 * (2 * (int64_t)K);         // double [2 buffers][K]
  c.total = up4l(o);
  return c;
}

// ---- length bonus, coverage term, end detection (semantics in include/ssasr.h, ssasr_beam_terms) ------------------
// TERMS true: the same loop with beta added to every non-<EOS> candidate, eta * (cov' - cov) to every candidate of a
// parent, and the stop rule after the selection.  Coverage state, per live hypothesis g: cum_g [T] floats in the
// workspace slice behind everything else (T goes to 16,384), double-buffered like the Speller state -- phase 3 adds
// the step's attention row to the parent's row in place and counts, phase 11 copies the parent's row into the new
// slot's row of the other buffer -- and cov_g, the step's cov' and the step's increments in LDS (K ints / floats).
// eta == 0: no coverage state, the slice is the plain / CTC one.  n_steps is written by every instantiation.
struct TermsDev {
  float beta, eta, tau, delta;            // delta < 0: no end detection
  int32_t* n_steps;
};

// floats of one utterance's coverage block: cum, 2 buffers x K rows of up4(T)
__host__ __device__ inline int64_t cov_ws_floats(const BeamWs& m, int K) { return 2 * (int64_t)K * m.Tp; }

// floats of one utterance's slice of the beam search's workspace: the plain or the CTC form's blocks, then the coverage
// block.  The kernel's slice stride and the three size queries.
__host__ __device__ inline int64_t beam_slice_floats(const BeamWs& m, int K, int T, bool ctc, bool cover) {
  return (ctc ? ctc_ws_map(m, K, T).total : m.total) + (cover ? cov_ws_floats(m, K) : 0);
}

// ---- character graph (semantics in include/ssasr.h, ssasr_decode_beam_graph) ---------------------------------------
// GRAPH true: the same loop with weight * arc[state_b][v] (fin[state_b] on the <EOS> lane) added last to every
// candidate of parent b, candidates at -inf never chosen.  Per live hypothesis g: state(g) (int32) and G(g) (double) in
// LDS by step parity, re-parented with the beam like the coverage counts; the finished entries' G + fin beside
// fin_score.  The only reads of the tables are one row of arc (4 V bytes) per live hypothesis and step in phase 8 and,
// once the winners are known, next and arc of the <= K picked candidates and fin of the step's finished ones, a lane
// each.  Every state taken from next is clamped to [0, S - 1] (start is checked by the entry): a malformed table gives
// wrong scores, never a read outside the tables.  The workspace slice is the form's without a graph.
struct GraphDev {
  const int32_t* next;                    // [S][V]
  const float *arc, *fin;                 // [S][V], [S]
  int S, start;
  float weight;                           // > 0 in every GRAPH instantiation
  float* graph_scores;                    // [N][K], output order
};

// The graph term of candidate (b, lane) for the wave that owns a hypothesis in `state`: weight * arc[state][lane], or
// weight * fin[state] on the <EOS> lane, as ONE float product (the caller adds it last).  A lane >= V reads nothing.
__device__ __forceinline__ float graph_term(const GraphDev& gd, int state, int V, int eos) {
  const int lane = threadIdx.x & 63;
  float g = 0.f;
  if (lane == eos) g = gd.fin[state];
  else if (lane < V) g = gd.arc[(int64_t)state * V + lane];
  return __fmul_rn(gd.weight, g);
}

constexpr int kCtcAhead = 4;              // frames whose loads a lattice loop issues before it needs the first

// log(exp(a) + exp(b))
__device__ __forceinline__ double log_add(double a, double b) {
  const double m = fmax(a, b);
  if (m == (double)-INFINITY) return m;
  return m + (double)logf(1.f + expf((float)(fmin(a, b) - m)));
}

// phi_t of a prefix extended by a character: what may precede that character's first frame t, from the parent's
// lattice at t - 1 (rep: the character repeats the parent's last one, so a blank has to lie between)
__device__ __forceinline__ double ctc_phi(double pb, double pn, bool rep) { return rep ? pb : log_add(pb, pn); }

// this lane's log_softmax(row)[lane]; called by a whole wave (V <= 64); what a lane >= V gets is no score
__device__ float log_softmax_lane(const float* row, int V) {
  const int lane = threadIdx.x & 63;
  const float x = lane < V ? row[lane] : -INFINITY;
  const float xm = wave_max(x);
  const float xs = wave_sum(lane < V ? expf(x - xm) : 0.f);
  return x - xm - logf(xs);
}

// psi(g . v), the CTC prefix score of the parent's prefix extended by v, from the parent's lattice rows alone:
// logsumexp over t of phi_t + lp[t][v], as a running maximum and a sum of float exps of differences from it.
// empty: the parent is the empty prefix (phi_0 = 0, otherwise -inf).  Called per lane with its own v.
__device__ double ctc_prefix_score(const float* lp, const double* gn, const double* gb, int len, int v, bool empty,
                                   bool rep) {
  double mx = -INFINITY, sum = 0.0;
  if (empty) {
    mx = (double)lp[v];
    sum = 1.0;
  }
  for (int t0 = 1; t0 < len; t0 += kCtcAhead) {
    double pb[kCtcAhead], pn[kCtcAhead];
    float l[kCtcAhead];
#pragma unroll
    for (int i = 0; i < kCtcAhead; ++i) {
      const int t = min(t0 + i, len - 1);
      pb[i] = gb[t - 1];
      pn[i] = gn[t - 1];
      l[i] = lp[(int64_t)t * 64 + v];
    }
#pragma unroll
    for (int i = 0; i < kCtcAhead; ++i) {
      if (t0 + i >= len) break;
      const double x = ctc_phi(pb[i], pn[i], rep) + (double)l[i];
      if (x > mx) {
        sum = sum * (double)expf((float)(mx - x)) + 1.0;
        mx = x;
      } else if (x > (double)-INFINITY) {
        sum += (double)expf((float)(x - mx));
      }
    }
  }
  return mx == (double)-INFINITY ? mx : mx + (double)logf((float)sum);
}

// The lattice rows of the parent's prefix extended by v, by the standard recursion, for one thread:
// hn[t] = log_add(hn[t-1], phi_t) + lp[t][v], hb[t] = log_add(hb[t-1], hn[t-1]) + lp[t][blank].
__device__ void ctc_extend(const float* lp, const double* pn0, const double* pb0, double* hn, double* hb, int len,
                           int v, int blank, bool empty, bool rep) {
  double n_ = empty ? (double)lp[v] : (double)-INFINITY, b_ = -INFINITY;
  hn[0] = n_;
  hb[0] = b_;
  for (int t0 = 1; t0 < len; t0 += kCtcAhead) {
    double pb[kCtcAhead], pn[kCtcAhead];
    float lv[kCtcAhead], l0[kCtcAhead];
#pragma unroll
    for (int i = 0; i < kCtcAhead; ++i) {
      const int t = min(t0 + i, len - 1);
      pb[i] = pb0[t - 1];
      pn[i] = pn0[t - 1];
      lv[i] = lp[(int64_t)t * 64 + v];
      l0[i] = lp[(int64_t)t * 64 + blank];
    }
#pragma unroll
    for (int i = 0; i < kCtcAhead; ++i) {
      if (t0 + i >= len) break;
      const double nn = log_add(n_, ctc_phi(pb[i], pn[i], rep)) + (double)lv[i];
      b_ = log_add(b_, n_) + (double)l0[i];
      n_ = nn;
      hn[t0 + i] = n_;
      hb[t0 + i] = b_;
    }
  }
}

// CTC false: ssasr_decode_beam's kernel (cd unread).  CTC true: the same loop with the candidates scored
// score_b + (1 - lambda) * log_softmax(asr) + lambda * (psi(h) - psi(g)) + lm_weight * log_softmax(lm), candidates
// at -inf never chosen; only the prologue and phases 8 to 11 differ.  TERMS false: td.n_steps alone is read.
// GRAPH false: gd is unread.
template <bool CTC, bool TERMS, bool GRAPH = false>
__global__ __launch_bounds__(kThreads) void decode_beam_kernel(BeamDev bd, CtcDev cd, TermsDev td, GraphDev gd) {
  __shared__ float cand[kMaxBeam * 64];            // score_b + row_b[v]; NaN: struck out
  __shared__ float score[2][kMaxBeam];             // live hypotheses' scores, by step parity
  __shared__ float redv[kWaves];
  __shared__ int redi[kWaves];
  __shared__ int pick[kMaxBeam];                   // chosen flat indices, candidate order
  __shared__ float pick_score[kMaxBeam];
  __shared__ int par[kMaxBeam], chr[kMaxBeam];     // new live slots: parent slot, character
  __shared__ float fin_score[kMaxBeam];            // finished / capped hypotheses in (step, candidate order)
  __shared__ int fin_len[kMaxBeam], fin_par[kMaxBeam];
  __shared__ int counts[TERMS ? 3 : 2];            // new live slots, finished hypotheses; TERMS: the stop rule fired
  __shared__ double cpsi[CTC ? kMaxBeam * 64 : 1]; // CTC: psi of the step's candidates
  __shared__ int lastc[2][CTC ? kMaxBeam : 1];     // CTC: the live hypotheses' last characters, by step parity
  __shared__ int cov[2][TERMS ? kMaxBeam : 1];     // coverage: the live hypotheses' counts, by step parity
  __shared__ int cov_new[TERMS ? kMaxBeam : 1];    // coverage: cov' of the step's parents
  __shared__ float cov_inc[TERMS ? kMaxBeam : 1];  // coverage: eta * (cov' - cov) of the step's parents
  __shared__ int gstate[2][GRAPH ? kMaxBeam : 1];  // graph: the live hypotheses' states, by step parity
  __shared__ double gsum[2][GRAPH ? kMaxBeam : 1]; // graph: the live hypotheses' G, by step parity
  __shared__ double fin_graph[GRAPH ? kMaxBeam : 1];   // graph: G (+ fin when ended) of the fin_score entries

  const InferDev& p = bd.in;
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = p.T, E = p.E, A = p.A, D = p.D, V = p.V, Hl = p.lm.H, K = bd.K, S = p.max_steps;
  const BeamWs m = beam_ws_map(K, T, E, A, D, Hl, S);
  const CtcWs cm = ctc_ws_map(m, K, T);
  const bool cover = TERMS && td.eta != 0.f;
  float* ws = bd.ws + (int64_t)n * beam_slice_floats(m, K, T, CTC, cover);
  const StepWs w = step_ws(m, ws, K, D + E);
  int32_t* bp = reinterpret_cast<int32_t*>(ws + m.bp);
  const int Sz = w.Sz, Tp = w.Tp, XI = w.XI;

  const int len = min(max(p.enc_len[n], 1), T);      // frames this utterance attends over
  const float* feat = p.feat + (int64_t)n * T * E;
  float* comp = p.comp + (int64_t)n * T * A;
  int32_t* chars = p.chars + (int64_t)n * K * S;
  int32_t* n_chars = p.n_chars + (int64_t)n * K;
  float* hyp_scores = bd.hyp_scores + (int64_t)n * K;

  // comp, and one live hypothesis: zero states, score 0, <SOS> = 0 as the input character
  float* cur = ws + m.st;
  float* nxt = cur + (int64_t)K * Sz;
  decode_prologue(p, w, feat, comp, len, cur, 1);
  if (tid == 0) score[0][0] = 0.f;
  // CTC: lp = log_softmax(ctc_head(feat)) of this utterance's frames, the head against the frames as vectors, then a
  // wave per row; the empty prefix: gamma_n = -inf, gamma_b[t] = lp[0][blank] + .. + lp[t][blank], psi = 0
  float* lp = ws + cm.lp;
  double* gcur = reinterpret_cast<double*>(ws + cm.gam);
  double* gnxt = gcur + (int64_t)K * 2 * T;
  double* psi_cur = reinterpret_cast<double*>(ws + cm.psi);
  double* psi_nxt = psi_cur + K;
  if constexpr (CTC) {
    matmat(cd.w, E, feat, E, E, nullptr, 0, nullptr, 0, 0, cd.b, nullptr, V, 0, lp, 64, len);
    phase_sync();
    for (int t = wave; t < len; t += kWaves) {
      float* row = lp + (int64_t)t * 64;
      const float x = lane < V ? row[lane] : -INFINITY;
      const float xm = wave_max(x);
      const float xs = wave_sum(lane < V ? expf(x - xm) : 0.f);
      const double l = (double)xm + (double)logf(xs);
      if (lane < V) row[lane] = (float)((double)x - l);
    }
    for (int t = tid; t < len; t += kThreads) gcur[t] = -INFINITY;
    phase_sync();
    if (tid == 0) {
      double s = 0.0;
      for (int t = 0; t < len; ++t) {
        s += (double)lp[(int64_t)t * 64 + cd.blank];
        gcur[T + t] = s;
      }
      psi_cur[0] = 0.0;
    }
  }
  // coverage: the empty prefix has attended to nothing
  float* ccur = ws + (CTC ? cm.total : m.total);
  float* cnxt = ccur + (int64_t)K * Tp;
  if constexpr (TERMS) {
    if (cover) {
      for (int t = tid; t < len; t += kThreads) ccur[t] = 0.f;
      if (tid == 0) cov[0][0] = 0;
    }
  }
  // graph: the empty prefix is in the start state with G = 0
  if constexpr (GRAPH) {
    if (tid == 0) {
      gstate[0][0] = gd.start;
      gsum[0][0] = 0.0;
    }
  }
  phase_sync();

  int live = 1, nfin = 0, step = 0;
  for (; step < S && live > 0; ++step) {
    const float* sc = score[step & 1];
    float* sc_new = score[(step + 1) & 1];
    // 1 to 7: the step's logit rows of the live hypotheses.  Coverage: the attention row is normalised, added to the
    // parent's cum in place and counted in one pass: cov' = frames with cum' > tau
    speller_step(p, w, feat, comp, len, cur, live, [&](int b, float* row, float sum) {
      if constexpr (TERMS) {
        if (cover) {
          float* cum = ccur + (int64_t)b * Tp;
          float cnt = 0.f;                           // an integer <= 16,384: exact, whatever the order
          for (int t = lane; t < len; t += 64) {
            const float a = row[t] / sum;
            row[t] = a;
            const float c = cum[t] + a;
            cum[t] = c;
            cnt += c > td.tau ? 1.f : 0.f;
          }
          const int cn = (int)wave_sum(cnt);
          if (lane == 0) {
            cov_new[b] = cn;
            cov_inc[b] = td.eta * (float)(cn - cov[step & 1][b]);
          }
          return;
        }
      }
      normalise_row(row, sum, len);
    });
    const float *lg = w.lg, *lmlg = w.lmlg;
    // 8: candidates score_b + log_softmax(asr) + lm_weight * log_softmax(lm), a wave per hypothesis
    if constexpr (CTC) {
      // lane v owns candidate (b, v) and runs the frame loop over its parent's lattice rows
      for (int b = wave; b < live; b += kWaves) {
        const float a = log_softmax_lane(lg + b * 64, V);
        const float l = Hl ? log_softmax_lane(lmlg + b * 64, V) : 0.f;
        const double *gn = gcur + (int64_t)b * 2 * T, *gb = gn + T;
        const int v = min(lane, V - 1);
        double ps = ctc_prefix_score(lp, gn, gb, len, v, step == 0, step > 0 && v == lastc[step & 1][b]);
        if (v == p.eos) ps = log_add(gn[len - 1], gb[len - 1]);
        if (v == cd.blank) ps = -INFINITY;
        cpsi[b * 64 + lane] = ps;
        float fin = (1.f - cd.lambda) * a + cd.lambda * (float)(ps - psi_cur[b]);
        if (Hl) fin += p.lm_weight * l;
        fin += sc[b];
        if constexpr (TERMS) {
          if (lane != p.eos) fin += td.beta;
          if (cover) fin += cov_inc[b];
        }
        if constexpr (GRAPH) fin = __fadd_rn(fin, graph_term(gd, gstate[step & 1][b], V, p.eos));
        cand[b * 64 + lane] = (lane < V && fin == fin) ? fin : -INFINITY;
      }
    } else {
      for (int b = wave; b < live; b += kWaves) {
        float fin = score_row(lg + b * 64, Hl ? lmlg + b * 64 : nullptr, V, p.lm_weight) + sc[b];
        if constexpr (TERMS) {
          if (lane != p.eos) fin += td.beta;
          if (cover) fin += cov_inc[b];
        }
        if constexpr (GRAPH) fin = __fadd_rn(fin, graph_term(gd, gstate[step & 1][b], V, p.eos));
        cand[b * 64 + lane] = (lane < V && fin == fin) ? fin : -INFINITY;      // a NaN is never chosen before a number
      }
    }
    __syncthreads();
    // 9: the W best, in order: W rounds of a block-wide arg-max, ties to the lower flat index
    int width = min(K - nfin, live * V);
    if constexpr (CTC || GRAPH) {                    // a candidate at -inf is never chosen
      int finite = 0;
      for (int c0 = 0; c0 < live * 64; c0 += kThreads)
        finite += __syncthreads_count(c0 + tid < live * 64 && cand[min(c0 + tid, live * 64 - 1)] > -INFINITY);
      width = min(width, finite);
    }
    for (int i = 0; i < width; ++i) {
      float bv = -INFINITY;
      int bi = kNone;
      for (int c = tid; c < live * 64; c += kThreads) {
        const float v = cand[c];
        if ((c & 63) < V && v == v && (bi == kNone || v > bv)) {
          bv = v;
          bi = c;
        }
      }
      const float wv = wave_max(bv);
      const int wi = (int)-wave_max(-(float)((bi != kNone && bv == wv) ? bi : kNone));    // indices < 2^24: exact
      if (lane == 0) {
        redv[wave] = wv;
        redi[wave] = wi;
      }
      __syncthreads();
      float best = -INFINITY;
      int at = kNone;
      for (int w = 0; w < kWaves; ++w) {
        const float v = redv[w];
        const int c = redi[w];
        if (c != kNone && (at == kNone || v > best || (v == best && c < at))) {
          best = v;
          at = c;
        }
      }
      at = min(at, live * 64 - 1);                  // every round has a candidate left (width <= live * V)
      if (tid == 0) {
        pick[i] = at;
        pick_score[i] = best;
        cand[at] = __builtin_nanf("");
      }
      __syncthreads();
    }
    // 10: <EOS> candidates finish their parent's prefix; the others are the new live set, in candidate order
    if (tid == 0) {
      int nl = 0, nf = nfin;
      for (int i = 0; i < width; ++i) {
        const int b = pick[i] >> 6, v = pick[i] & 63;
        if (v == p.eos) {
          fin_score[nf] = pick_score[i];
          fin_len[nf] = step;                       // a hypothesis live at step s has s characters
          fin_par[nf] = b;
          ++nf;
        } else {
          par[nl] = b;
          chr[nl] = v;
          sc_new[nl] = pick_score[i];
          bp[(int64_t)step * K + nl] = b | (v << 8);
          if constexpr (CTC) {
            psi_nxt[nl] = cpsi[pick[i]];
            lastc[(step + 1) & 1][nl] = v;
          }
          if constexpr (TERMS) {
            if (cover) cov[(step + 1) & 1][nl] = cov_new[b];
          }
          ++nl;
        }
      }
      counts[0] = nl;
      counts[1] = nf;
      if constexpr (TERMS) {                         // the stop rule: the best live score is below the best finished - delta
        int stop = 0;
        if (td.delta >= 0.f && nf > 0 && nl > 0) {
          float ml = sc_new[0], mf = fin_score[0];
          for (int j = 1; j < nl; ++j) ml = fmaxf(ml, sc_new[j]);
          for (int j = 1; j < nf; ++j) mf = fmaxf(mf, fin_score[j]);
          stop = ml < mf - td.delta;
        }
        counts[2] = stop;
      }
    }
    __syncthreads();
    const int nl = counts[0];
    // graph: a new slot's state and G from next and arc of its picked candidate, the step's finished entries' G + fin;
    // a lane each, so the up to K look-ups are in flight together (the two ranges lie in different waves)
    if constexpr (GRAPH) {
      const int* gs = gstate[step & 1];
      const double* gG = gsum[step & 1];
      if (tid < nl) {
        const int b = par[tid];
        const int64_t at = (int64_t)gs[b] * V + chr[tid];
        gstate[(step + 1) & 1][tid] = min(max(gd.next[at], 0), gd.S - 1);
        gsum[(step + 1) & 1][tid] = gG[b] + (double)gd.arc[at];
      } else if (tid >= 64 && tid - 64 < counts[1] - nfin) {
        const int j = nfin + tid - 64, b = fin_par[j];
        fin_graph[j] = gG[b] + (double)gd.fin[gs[b]];
      }
    }
    nfin = counts[1];
    if constexpr (TERMS) {
      if (counts[2]) {                               // the live hypotheses are abandoned prefixes: discarded, not emitted
        live = 0;
        ++step;
        break;
      }
    }
    // 11: a new slot's state is its parent's row, copied into the other buffer; its inputs are its character's
    for (int i = tid; i < nl * (Sz / 4); i += kThreads) {
      const int j = i / (Sz / 4), o = i % (Sz / 4);
      reinterpret_cast<float4*>(nxt + (int64_t)j * Sz)[o] = reinterpret_cast<const float4*>(cur + (int64_t)par[j] * Sz)[o];
    }
    for (int i = tid; i < nl * D; i += kThreads) {
      const int j = i / D, u = i % D;
      w.xin[(int64_t)j * XI + u] = p.embed[(int64_t)chr[j] * D + u];
    }
    for (int i = tid; i < nl * Hl; i += kThreads) {
      const int j = i / Hl, u = i % Hl;
      w.lmx[(int64_t)j * Hl + u] = p.lm.emb[(int64_t)chr[j] * Hl + u];
    }
    if constexpr (TERMS) {                           // and its coverage row is its parent's cum'
      if (cover) {
        const int n4 = up4(len) / 4;
        for (int i = tid; i < nl * n4; i += kThreads) {
          const int j = i / n4, o = i % n4;
          reinterpret_cast<float4*>(cnxt + (int64_t)j * Tp)[o] =
              reinterpret_cast<const float4*>(ccur + (int64_t)par[j] * Tp)[o];
        }
        float* c = ccur;
        ccur = cnxt;
        cnxt = c;
      }
    }
    if constexpr (CTC) {                             // and its lattice rows are its parent's, advanced by its character
      if (tid < nl) {
        const double* pn = gcur + (int64_t)par[tid] * 2 * T;
        double* hn = gnxt + (int64_t)tid * 2 * T;
        ctc_extend(lp, pn, pn + T, hn, hn + T, len, chr[tid], cd.blank, step == 0,
                   step > 0 && chr[tid] == lastc[step & 1][par[tid]]);
      }
      double* g = gcur;
      gcur = gnxt;
      gnxt = g;
      g = psi_cur;
      psi_cur = psi_nxt;
      psi_nxt = g;
    }
    phase_sync();
    float* t = cur;
    cur = nxt;
    nxt = t;
    live = nl;
  }
  // the cap: what is still live is emitted as it stands (no <EOS> term), after the finished ones of equal score
  if (tid == 0) {
    const float* sc = score[step & 1];
    for (int j = 0; j < live; ++j) {
      fin_score[nfin + j] = sc[j];
      fin_len[nfin + j] = step;
      fin_par[nfin + j] = j;
      if constexpr (GRAPH) fin_graph[nfin + j] = gsum[step & 1][j];      // no fin term, as no <EOS> term
    }
  }
  const int total = nfin + live;                    // <= K: finished + width == K at every step, live <= width
  for (int64_t i = tid; i < (int64_t)K * S; i += kThreads) chars[i] = 0;
  if (tid < K) {
    n_chars[tid] = 0;
    hyp_scores[tid] = 0.f;
    if constexpr (GRAPH) gd.graph_scores[(int64_t)n * K + tid] = 0.f;
  }
  if (tid == 0) bd.n_hyps[n] = total;
  if (tid == 0 && td.n_steps) td.n_steps[n] = step;  // loop iterations executed
  phase_sync();
  // output order: score descending, ties to the earlier entry of the (step, candidate order) list
  if (tid < total) {
    const float s = fin_score[tid];
    int rank = 0;
    for (int j = 0; j < total; ++j) rank += (fin_score[j] > s || (fin_score[j] == s && j < tid)) ? 1 : 0;
    hyp_scores[rank] = s;
    if constexpr (GRAPH) gd.graph_scores[(int64_t)n * K + rank] = (float)fin_graph[tid];   // rounded once from double
    n_chars[rank] = fin_len[tid];
    int slot = fin_par[tid];
    for (int pos = fin_len[tid] - 1; pos >= 0; --pos) {         // trace the back-pointers
      const int e = bp[(int64_t)pos * K + slot];
      chars[(int64_t)rank * S + pos] = e >> 8;
      slot = e & 255;
    }
  }
}

// ---- sampled decoding (semantics in include/ssasr.h, ssasr_decode_sample) ------------------------------------------
// decode_sample_kernel: the loop of decode_greedy_kernel for K independent samples of one utterance in ONE workgroup,
// with decode_beam_kernel's layout -- a workgroup owns an utterance for the whole loop, exchanges nothing and never
// spins; comp is computed once; every weight matrix and feat are streamed once per step for all of the utterance's
// samples; per-sample state and intermediates are in the workspace slice, writer and reader phases a phase_sync()
// apart.  There is no selection and no re-parenting: a slot's state is kept ONCE and updated in place, its characters
// go straight to the output row, and LDS holds the slots' flags, last characters and two running sums.
// Finished slots stay where they are.  The products run over slots 0 .. hi - 1, hi being one past the highest live
// slot; what a finished slot below hi computes is discarded (its flag is down: it draws nothing, writes nothing and
// is fed nothing).  matmat_n, context_partial and the updates give a vector the same bits wherever it lies and however
// many lie beside it, so a sample does not depend on the other slots.  Why not compact: a pass of matmat holds kHyps
// vectors against the streamed rows, so at K <= kHyps a dead slot costs FMAs in a pass that runs anyway, and moving
// a live slot's state rows into a hole would cost a copy phase and a slot map for the outputs; trimming to hi sheds
// the passes that a finished tail would cost at K > kHyps.
struct SampleDev {
  BeamDev b;
  const float* uniforms;                  // [N][K][S]
  float tau;
  float* logq;                            // [N][K] or nullptr
};

__global__ __launch_bounds__(kThreads) void decode_sample_kernel(SampleDev sd) {
  __shared__ int alive[kMaxBeam], chr[kMaxBeam], nch[kMaxBeam];
  __shared__ float score[kMaxBeam], logq[kMaxBeam];  // sums over the drawn characters: row[v], log q(v)

  const InferDev& p = sd.b.in;
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = p.T, E = p.E, A = p.A, D = p.D, V = p.V, Hl = p.lm.H, K = sd.b.K, S = p.max_steps;
  const BeamWs m = sample_ws_map(K, T, E, A, D, Hl);
  float* ws = sd.b.ws + (int64_t)n * m.total;
  const StepWs w = step_ws(m, ws, K, D + E);
  float *st = ws + m.st, *lg = w.lg, *lmlg = w.lmlg;
  const int XI = w.XI;

  const int len = min(max(p.enc_len[n], 1), T);      // frames this utterance attends over
  const float* feat = p.feat + (int64_t)n * T * E;
  float* comp = p.comp + (int64_t)n * T * A;
  int32_t* chars = p.chars + (int64_t)n * K * S;
  const float* uni = sd.uniforms + (int64_t)n * K * S;

  // comp, and K samples: zero states, <SOS> = 0 as the input character
  decode_prologue(p, w, feat, comp, len, st, K);
  for (int64_t i = tid; i < (int64_t)K * S; i += kThreads) chars[i] = 0;
  if (tid < K) {
    alive[tid] = 1;
    nch[tid] = S;                                    // a sample the cap ends has max_steps characters
    score[tid] = 0.f;
    logq[tid] = 0.f;
  }
  phase_sync();

  int hi = K;                                        // one past the highest live slot
  for (int step = 0; step < S && hi > 0; ++step) {
    // 1 to 7: the logit rows of slots 0 .. hi - 1
    speller_step(p, w, feat, comp, len, st, hi, [&](int, float* row, float sum) { normalise_row(row, sum, len); });
    // 8: the draw, a wave per live sample: z = row / tau, e = exp(z - max z), the first v whose running sum of e
    // exceeds u * total (V - 1 when none does); the sums run in index order, the same in every lane
    for (int b = wave; b < hi; b += kWaves) {
      if (!alive[b]) continue;
      const float fin = score_row(lg + b * 64, Hl ? lmlg + b * 64 : nullptr, V, p.lm_weight);
      const float z = lane < V ? fin / sd.tau : -INFINITY;
      const float zm = wave_max(z);
      const float e = lane < V ? expf(z - zm) : 0.f;
      float total = 0.f;
      for (int v = 0; v < V; ++v) total += __shfl(e, v, 64);
      const float target = uni[(int64_t)b * S + step] * total;
      float run = 0.f;
      int pick = V - 1;
      for (int v = 0; v < V; ++v) {
        run += __shfl(e, v, 64);
        if (run > target) {
          pick = v;
          break;
        }
      }
      const float rv = __shfl(fin, pick, 64), zv = __shfl(z, pick, 64);
      if (lane == 0) {
        score[b] += rv;
        logq[b] += zv - zm - logf(total);
        if (pick == p.eos) {                         // <EOS> ends the sample and is not part of the text
          alive[b] = 0;
          nch[b] = step;
        } else {
          chars[(int64_t)b * S + step] = pick;
          chr[b] = pick;
        }
      }
    }
    __syncthreads();
    // 9: the live slots' next inputs are their characters' embeddings
    int top = 0;
    for (int b = 0; b < hi; ++b) top = alive[b] ? b + 1 : top;
    hi = top;
    for (int i = tid; i < hi * D; i += kThreads) {
      const int j = i / D, u = i % D;
      if (alive[j]) w.xin[(int64_t)j * XI + u] = p.embed[(int64_t)chr[j] * D + u];
    }
    for (int i = tid; i < hi * Hl; i += kThreads) {
      const int j = i / Hl, u = i % Hl;
      if (alive[j]) w.lmx[(int64_t)j * Hl + u] = p.lm.emb[(int64_t)chr[j] * Hl + u];
    }
    phase_sync();
  }
  if (tid < K) {
    p.n_chars[(int64_t)n * K + tid] = nch[tid];
    sd.b.hyp_scores[(int64_t)n * K + tid] = score[tid];
    if (sd.logq) sd.logq[(int64_t)n * K + tid] = logq[tid];
  }
  if (tid == 0) sd.b.n_hyps[n] = K;
}

// One CharLM.forward (src/charlm.py:46-57) for B rows, a workgroup per row.
struct LmStepDev {
  LmDev lm;
  int V;
  const int32_t* x;
  const float *h1, *h2;
  float *out, *h1_out, *h2_out;
};

__global__ __launch_bounds__(kThreads) void charlm_step_kernel(LmStepDev p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int b = blockIdx.x, H = p.lm.H;
  float *x = lds, *h1 = x + H, *h2 = h1 + H, *gi = h2 + H, *gh = gi + 3 * H;
  const int id = min(max(p.x[b], 0), p.V - 1);
  copy_row(x, p.lm.emb + (int64_t)id * H, H);
  copy_row(h1, p.h1 + (int64_t)b * H, H);
  copy_row(h2, p.h2 + (int64_t)b * H, H);
  __syncthreads();
  matvec(p.lm.w_ih1, H, x, H, nullptr, 0, nullptr, 0, p.lm.b_ih1, nullptr, 3 * H, 0, gi);
  matvec(p.lm.w_hh1, H, h1, H, nullptr, 0, nullptr, 0, p.lm.b_hh1, nullptr, 3 * H, 0, gh);
  __syncthreads();
  gru_update(gi, gh, 0, h1, 0, H, 1);
  __syncthreads();
  matvec(p.lm.w_ih2, H, h1, H, nullptr, 0, nullptr, 0, p.lm.b_ih2, nullptr, 3 * H, 0, gi);
  matvec(p.lm.w_hh2, H, h2, H, nullptr, 0, nullptr, 0, p.lm.b_hh2, nullptr, 3 * H, 0, gh);
  __syncthreads();
  gru_update(gi, gh, 0, h2, 0, H, 1);
  __syncthreads();
  matvec(p.lm.w_out, H, h2, H, nullptr, 0, nullptr, 0, p.lm.b_out, nullptr, p.V, 0, p.out + (int64_t)b * p.V);
  copy_row(p.h1_out + (int64_t)b * H, h1, H);
  copy_row(p.h2_out + (int64_t)b * H, h2, H);
}

// ---- CTC prefix beam search with the CharLM inside the search (include/ssasr.h, "CTC decoding with an LM") ----------
// BUILD-DEFINED.  ctc_prefix.h's frame body (the one ctc.hip's ctc_prefix_beam_kernel runs) with CtcLmTerm, at this
// file's kThreads: the term is here because the LM step is this file's helpers (matmat / gru_update / score_row).
// g_b / g_n stay pure CTC masses; a member also carries, in the body's acc, L (double, the LM's log-probability of its
// text) and a SLOT: lmrow[slot] in LDS is the LM's log-softmax row after the text, st[slot] in the workspace its two
// GRU rows.  A kept member keeps its slot; a new extension takes a slot no kept member holds.  A frame's new members
// step together in after_commit: their parents' states are gathered into `stage` (all of them, before any slot is
// overwritten), stepped kHyps at a time with the gate rows in the workspace, and scattered to their slots.  With
// lm.H == 0 (lm_weight == 0) no step runs and no slot is read.

// one utterance's float blocks of the workspace (floats; every block starts on 16 bytes)
struct CtcLmWs {
  int64_t st, stage, lmx, gi, gh, lmlg, total;
};
__host__ __device__ inline CtcLmWs ctc_lm_ws_map(int K, int H) {
  CtcLmWs m;
  const int ns = K < kHyps ? K : kHyps;
  int64_t o = 0;
  m.st = o; o += (int64_t)K * 2 * H;          // [slot][h1 | h2]
  m.stage = o; o += (int64_t)K * 2 * H;       // the frame's new members: their parents' states, stepped in place
  m.lmx = o; o += (int64_t)ns * H;            // the kHyps hypotheses in flight: embeddings, gate rows, output rows
  m.gi = o; o += (int64_t)ns * 3 * H;
  m.gh = o; o += (int64_t)ns * 3 * H;
  m.lmlg = o; o += H ? ns * 64 : 0;
  m.total = o;
  return m;
}

struct CtcLmDev {
  ctc_prefix::Args d;
  int eos;
  float lm_weight, length_bonus;
  LmDev lm;                  // H == 0: no LM term
  float* fws;                // [B][ctc_lm_ws_map(K, H).total]
  int32_t* lm_frames;        // [B] frames that ran an LM step (tools/ctc_lm_time.py)
  float *ctc_scores, *lm_scores;   // [B][K]
};

// One CharLM step (speller_step's LM phases) for n <= kHyps hypotheses: st holds their (h1 | h2) rows 2 H apart and
// is updated in place, lmx the embeddings of the characters fed; leaves the output rows in lmlg, 64 apart.
__device__ void ctc_lm_step(const LmDev& lm, int V, float* st, const float* lmx, float* gi, float* gh, float* lmlg,
                            int n) {
  const int H = lm.H, Sz = 2 * H;
  float *h1 = st, *h2 = st + H;
  matmat(lm.w_ih1, H, lmx, H, H, nullptr, 0, nullptr, 0, 0, lm.b_ih1, nullptr, 3 * H, 0, gi, 3 * H, n);
  matmat(lm.w_hh1, H, h1, Sz, H, nullptr, 0, nullptr, 0, 0, lm.b_hh1, nullptr, 3 * H, 0, gh, 3 * H, n);
  phase_sync();
  gru_update(gi, gh, 3 * H, h1, Sz, H, n);
  phase_sync();
  matmat(lm.w_ih2, H, h1, Sz, H, nullptr, 0, nullptr, 0, 0, lm.b_ih2, nullptr, 3 * H, 0, gi, 3 * H, n);
  matmat(lm.w_hh2, H, h2, Sz, H, nullptr, 0, nullptr, 0, 0, lm.b_hh2, nullptr, 3 * H, 0, gh, 3 * H, n);
  phase_sync();
  gru_update(gi, gh, 3 * H, h2, Sz, H, n);
  phase_sync();
  matmat(lm.w_out, H, h2, Sz, H, nullptr, 0, nullptr, 0, 0, lm.b_out, nullptr, V, 0, lmlg, 64, n);
  phase_sync();
}

struct CtcLmTerm : ctc_prefix::Scored {
  struct Mem : ctc_prefix::ScoredMem {
    float lmrow[ctc_prefix::kMaxK][64];                      // [slot]: the LM's log-softmax row after the text
  };
  const CtcLmDev& a;
  float *st, *stage, *lmx, *gi, *gh, *lmlg;                  // the utterance's blocks of the workspace
  int lm_frames = 0;

  __device__ explicit CtcLmTerm(const CtcLmDev& dev)
      : Scored{dev.lm.H > 0, dev.length_bonus != 0.f, (double)dev.lm_weight, (double)dev.length_bonus, dev.ctc_scores,
               dev.lm_scores},
        a(dev) {
    const CtcLmWs m = ctc_lm_ws_map(dev.d.K, dev.lm.H);
    float* ws = dev.fws + (int64_t)blockIdx.x * m.total;
    st = ws + m.st; stage = ws + m.stage; lmx = ws + m.lmx; gi = ws + m.gi; gh = ws + m.gh; lmlg = ws + m.lmlg;
  }

  __device__ void init(Mem& m, int V) const {                // the empty text's row: <SOS> = 0 from zero states
    if (!on) return;
    const int tid = threadIdx.x, H = a.lm.H, Sz = 2 * H;
    for (int i = tid; i < Sz; i += kThreads) stage[i] = 0.f;
    for (int i = tid; i < H; i += kThreads) lmx[i] = a.lm.emb[i];
    phase_sync();
    ctc_lm_step(a.lm, V, stage, lmx, gi, gh, lmlg, 1);
    if (tid < 64) {
      const float r = score_row(lmlg, nullptr, V, 0.f);
      m.lmrow[0][tid] = tid < V ? r : 0.f;
    }
    for (int i = tid; i < Sz; i += kThreads) st[i] = stage[i];
    __threadfence_block();                                   // with the body's barrier: a phase_sync()
  }
  __device__ double step(const Mem& m, int cur, int u, int c) const { return (double)m.lmrow[m.slot[cur][u]][c]; }
  __device__ void keep(Mem&, int, int, int, int) const {}
  __device__ void inherit(Mem&, int, int, int, int, int) const {}
  // the new members' LM step
  template <class S>
  __device__ void after_commit(S& s, int cur, int nxt, int K, int V) {
    Mem& m = s.tm;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, H = a.lm.H, Sz = 2 * H;
    const int ne = on ? m.n_ext : 0;
    if (ne == 0) return;
    ++lm_frames;
    for (int i = tid; i < ne * Sz; i += kThreads) {          // every parent's state, before any slot is written
      const int e = i / Sz, u = (s.win[m.ext[e]] - K) / V;
      stage[i] = st[(int64_t)m.slot[cur][u] * Sz + i % Sz];
    }
    for (int e0 = 0; e0 < ne; e0 += kHyps) {
      const int nb = min(kHyps, ne - e0);
      for (int i = tid; i < nb * H; i += kThreads) {
        const int c = (s.win[m.ext[e0 + i / H]] - K) % V;
        lmx[i] = a.lm.emb[(int64_t)c * H + i % H];
      }
      phase_sync();
      ctc_lm_step(a.lm, V, stage + (int64_t)e0 * Sz, lmx, gi, gh, lmlg, nb);
      for (int e = wave; e < nb; e += kWaves) {
        const float r = score_row(lmlg + e * 64, nullptr, V, 0.f);
        m.lmrow[m.slot[nxt][m.ext[e0 + e]]][lane] = lane < V ? r : 0.f;
      }
    }
    for (int i = tid; i < ne * Sz; i += kThreads) st[(int64_t)m.slot[nxt][m.ext[i / Sz]] * Sz + i % Sz] = stage[i];
    phase_sync();
  }
  __device__ bool has_end() const { return a.eos >= 0; }
  __device__ double end(const Mem& m, int cur, int j) const { return (double)m.lmrow[m.slot[cur][j]][a.eos]; }
};

__global__ __launch_bounds__(kThreads) void ctc_prefix_beam_lm_kernel(CtcLmDev a) {
  __shared__ ctc_prefix::State<kThreads, CtcLmTerm> s;
  CtcLmTerm term(a);
  ctc_prefix::search(a.d, term, s);
  if (threadIdx.x == 0) a.lm_frames[blockIdx.x] = term.lm_frames;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// 0: not a usable parameter block
bool lm_ok(const ssasr_charlm* lm, LmDev& out) {
  if (!lm || lm->V <= 0 || lm->H <= 0 || lm->H % 4 != 0 || lm->H > 4096) return false;
  const float* ptrs[] = {lm->emb, lm->w_ih1, lm->w_hh1, lm->b_ih1, lm->b_hh1, lm->w_ih2, lm->w_hh2, lm->b_ih2,
                         lm->b_hh2, lm->w_out, lm->b_out};
  for (const float* q : ptrs)
    if (!q || !aligned16(q)) return false;
  out = LmDev{(int)lm->H, lm->emb, lm->w_ih1, lm->w_hh1, lm->b_ih1, lm->b_hh1, lm->w_ih2, lm->w_hh2, lm->b_ih2,
              lm->b_hh2, lm->w_out, lm->b_out};
  return true;
}

int allow_lds(const void* kernel, size_t bytes) {
  if (bytes > 64 * 1024)
    SSASR_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return SSASR_OK;
}

// the dimensions ssasr_decoder_fwd takes, with V <= 64 (one wave holds a score row) and K hypotheses an utterance
bool decode_dims_ok(int64_t N, int64_t K, int64_t T, int64_t E, int64_t A, int64_t D, int64_t V, int64_t Hl, int64_t S) {
  return N > 0 && N <= 0x7fffffff && K >= 1 && K <= kMaxBeam && T > 0 && T <= 16384 && E > 0 && E <= 8192 &&
         E % 4 == 0 && A > 0 && A <= 2048 && A % 4 == 0 && D > 0 && D <= 4096 && D % 16 == 0 && V > 0 && V <= 64 &&
         Hl >= 0 && Hl <= 4096 && Hl % 4 == 0 && S > 0 && S <= (1 << 20);
}

// What ssasr_infer and ssasr_beam (Desc) have in common: checks the dimensions for K hypotheses, the language
// model and the pointers, and fills p (all of it but scores / att).  false: not a usable description.
template <class Desc>
bool infer_dev(const Desc& d, int64_t K, InferDev& p) {
  if (d.lm && (!lm_ok(d.lm, p.lm) || d.lm->V != d.V)) return false;
  if (!decode_dims_ok(d.N, K, d.T, d.E, d.A, d.D, d.V, p.lm.H, d.max_steps) || d.eos < 0 || d.eos >= d.V) return false;
  const void* need[] = {d.feat, d.enc_len, d.comp, d.w_psi, d.b_psi, d.w_phi, d.w_ih1, d.w_hh1, d.b_ih1, d.b_hh1,
                        d.w_ih2, d.w_hh2, d.b_ih2, d.b_hh2, d.embed, d.w_ct, d.b_ct, d.chars, d.n_chars};
  for (const void* q : need)
    if (!q) return false;
  const void* vec[] = {d.feat, d.comp, d.w_psi, d.w_phi, d.w_ih1, d.w_hh1, d.w_ih2, d.w_hh2, d.embed, d.w_ct};
  for (const void* q : vec)
    if (!aligned16(q)) return false;
  p.T = (int)d.T; p.E = (int)d.E; p.A = (int)d.A; p.D = (int)d.D; p.V = (int)d.V;
  p.max_steps = (int)d.max_steps; p.eos = d.eos; p.lm_weight = d.lm ? d.lm_weight : 0.f;
  p.feat = d.feat; p.enc_len = d.enc_len; p.comp = d.comp; p.w_psi = d.w_psi; p.b_psi = d.b_psi; p.w_phi = d.w_phi;
  p.w_ih1 = d.w_ih1; p.w_hh1 = d.w_hh1; p.b_ih1 = d.b_ih1; p.b_hh1 = d.b_hh1;
  p.w_ih2 = d.w_ih2; p.w_hh2 = d.w_hh2; p.b_ih2 = d.b_ih2; p.b_hh2 = d.b_hh2;
  p.embed = d.embed; p.w_ct = d.w_ct; p.b_ct = d.b_ct;
  p.chars = d.chars; p.n_chars = d.n_chars;
  return true;
}

}  // namespace

extern "C" int ssasr_decode_greedy(const ssasr_infer* dp, void* stream) {
  InferDev p{};
  if (!dp || !infer_dev(*dp, 1, p) || !dp->scores) return SSASR_EARG;
  // what decode_beam_kernel keeps in its workspace is in LDS here
  const size_t bytes = sizeof(float) * (size_t)lds_map(p.T, p.E, p.A, p.D, p.lm.H).total;
  if (bytes > kMaxLds) return SSASR_EARG;
  p.scores = dp->scores; p.att = dp->att;
  if (const int rc = allow_lds(reinterpret_cast<const void*>(decode_greedy_kernel), bytes)) return rc;
  hipLaunchKernelGGL(decode_greedy_kernel, dim3((unsigned)dp->N), dim3(kThreads), bytes, (hipStream_t)stream, p);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}

extern "C" int64_t ssasr_decode_beam_ws_bytes(int64_t N, int64_t K, int64_t T, int64_t E, int64_t A, int64_t D,
                                              int64_t V, int64_t Hl, int64_t S) {
  return ssasr_decode_beam_ex_ws_bytes(N, K, T, E, A, D, V, Hl, S, 0, 0);
}

extern "C" int64_t ssasr_decode_beam_ctc_ws_bytes(int64_t N, int64_t K, int64_t T, int64_t E, int64_t A, int64_t D,
                                                  int64_t V, int64_t Hl, int64_t S) {
  return ssasr_decode_beam_ex_ws_bytes(N, K, T, E, A, D, V, Hl, S, 1, 0);
}

extern "C" int64_t ssasr_decode_beam_ex_ws_bytes(int64_t N, int64_t K, int64_t T, int64_t E, int64_t A, int64_t D,
                                                 int64_t V, int64_t Hl, int64_t S, int32_t ctc, int32_t coverage) {
  if (!decode_dims_ok(N, K, T, E, A, D, V, Hl, S)) return 0;
  const BeamWs m = beam_ws_map((int)K, (int)T, (int)E, (int)A, (int)D, (int)Hl, (int)S);
  return N * beam_slice_floats(m, (int)K, (int)T, ctc != 0, coverage != 0) * (int64_t)sizeof(float);
}

extern "C" int64_t ssasr_decode_sample_ws_bytes(int64_t N, int64_t K, int64_t T, int64_t E, int64_t A, int64_t D,
                                                int64_t V, int64_t Hl, int64_t S) {
  if (!decode_dims_ok(N, K, T, E, A, D, V, Hl, S)) return 0;
  return N * sample_ws_map((int)K, (int)T, (int)E, (int)A, (int)D, (int)Hl).total * (int64_t)sizeof(float);
}

namespace {

// What the K-hypothesis entries check alike and fill alike: the description (infer_dev), the workspace (there, on 16
// bytes, at least need(Hl) bytes: the entry's own size query) and the two per-hypothesis outputs.
template <class Need>
bool beam_dev(const ssasr_beam* dp, Need need, BeamDev& b) {
  if (!dp || !infer_dev(*dp, dp->K, b.in)) return false;
  const ssasr_beam& d = *dp;
  if (!d.ws || !aligned16(d.ws) || !d.hyp_scores || !d.n_hyps || d.ws_bytes < need(d, b.in.lm.H)) return false;
  b.K = (int)d.K; b.ws = d.ws; b.hyp_scores = d.hyp_scores; b.n_hyps = d.n_hyps;
  return true;
}

// ssasr_decode_beam_graph's graph arguments: the weight finite and >= 0, the output there, a graph's shape that of
// the search (looked at whenever one is passed) and, at a weight != 0, the graph and its tables there
bool graph_ok(const ssasr_char_graph* gp, float weight, const float* graph_scores, int64_t V) {
  if (!(std::isfinite(weight) && weight >= 0.f) || !graph_scores) return false;
  if (gp && (gp->V != V || gp->S < 1 || gp->S > (1 << 20) || gp->start < 0 || gp->start >= gp->S)) return false;
  return weight == 0.f || (gp && gp->next && gp->arc && gp->fin);
}

// ssasr_decode_beam (cp == nullptr), ssasr_decode_beam_ctc, ssasr_decode_beam_ex (tp != nullptr) and
// ssasr_decode_beam_graph (g.weight != 0: its checks are done)
int launch_beam(const ssasr_beam* dp, const ssasr_ctc_prefix* cp, const ssasr_beam_terms* tp, void* stream,
                const GraphDev& g = GraphDev{}) {
  TermsDev t{0.f, 0.f, 0.f, -1.f, nullptr};
  if (tp) {
    if (!std::isfinite(tp->length_bonus) || !std::isfinite(tp->coverage_weight) || tp->end_margin != tp->end_margin)
      return SSASR_EARG;
    if (tp->coverage_weight != 0.f && !(std::isfinite(tp->coverage_threshold) && tp->coverage_threshold > 0.f))
      return SSASR_EARG;
    t = TermsDev{tp->length_bonus, tp->coverage_weight, tp->coverage_weight != 0.f ? tp->coverage_threshold : 0.f,
                 tp->end_margin >= 0.f ? tp->end_margin : -1.f, tp->n_steps};
  }
  const bool terms = t.beta != 0.f || t.eta != 0.f || t.delta >= 0.f;
  BeamDev b{};
  const auto need = [&](const ssasr_beam& d, int Hl) {
    return ssasr_decode_beam_ex_ws_bytes(d.N, d.K, d.T, d.E, d.A, d.D, d.V, Hl, d.max_steps, cp ? 1 : 0, t.eta != 0.f);
  };
  if (!beam_dev(dp, need, b)) return SSASR_EARG;
  const ssasr_beam& d = *dp;
  CtcDev c{};
  if (cp) {
    if (!(cp->ctc_weight >= 0.f && cp->ctc_weight <= 1.f) || cp->blank < 0 || cp->blank >= d.V || cp->blank == d.eos)
      return SSASR_EARG;
    if (cp->ctc_weight > 0.f) {                     // weight 0: the head is unread, 0 * -inf is never formed
      if (!cp->w_ctc || !cp->b_ctc || !aligned16(cp->w_ctc)) return SSASR_EARG;
      c = CtcDev{cp->w_ctc, cp->b_ctc, cp->ctc_weight, cp->blank};
    }
  }
  // all terms off: the instantiations ssasr_decode_beam / ssasr_decode_beam_ctc launch
  // a graph: the TERMS forms alone are instantiated (with every term off they add 0 and stop nothing)
  const dim3 grid((unsigned)d.N), block(kThreads);
  if (g.weight != 0.f && c.w)
    hipLaunchKernelGGL((decode_beam_kernel<true, true, true>), grid, block, 0, (hipStream_t)stream, b, c, t, g);
  else if (g.weight != 0.f)
    hipLaunchKernelGGL((decode_beam_kernel<false, true, true>), grid, block, 0, (hipStream_t)stream, b, c, t, g);
  else if (c.w && terms)
    hipLaunchKernelGGL((decode_beam_kernel<true, true>), grid, block, 0, (hipStream_t)stream, b, c, t, g);
  else if (c.w)
    hipLaunchKernelGGL((decode_beam_kernel<true, false>), grid, block, 0, (hipStream_t)stream, b, c, t, g);
  else if (terms)
    hipLaunchKernelGGL((decode_beam_kernel<false, true>), grid, block, 0, (hipStream_t)stream, b, c, t, g);
  else
    hipLaunchKernelGGL((decode_beam_kernel<false, false>), grid, block, 0, (hipStream_t)stream, b, c, t, g);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}

}  // namespace

extern "C" int64_t ssasr_decode_beam_graph_ws_bytes(int64_t N, int64_t K, int64_t T, int64_t E, int64_t A, int64_t D,
                                                    int64_t V, int64_t Hl, int64_t S, int32_t ctc, int32_t coverage) {
  return ssasr_decode_beam_ex_ws_bytes(N, K, T, E, A, D, V, Hl, S, ctc, coverage);   // the graph state is in LDS
}

extern "C" int ssasr_decode_beam_graph(const ssasr_beam* dp, const ssasr_ctc_prefix* cp, const ssasr_beam_terms* tp,
                                       const ssasr_char_graph* gp, float graph_weight, float* graph_scores,
                                       void* stream) {
  if (!dp || !graph_ok(gp, graph_weight, graph_scores, dp->V)) return SSASR_EARG;
  if (graph_weight == 0.f) {                        // the tables are unread: ssasr_decode_beam_ex's launch, and G = 0
    if (const int rc = launch_beam(dp, cp, tp, stream)) return rc;
    SSASR_HIP(hipMemsetAsync(graph_scores, 0, sizeof(float) * (size_t)(dp->N * dp->K), (hipStream_t)stream));
    return SSASR_OK;
  }
  return launch_beam(dp, cp, tp, stream,
                     GraphDev{gp->next, gp->arc, gp->fin, gp->S, gp->start, graph_weight, graph_scores});
}

extern "C" int ssasr_decode_beam(const ssasr_beam* dp, void* stream) {
  return launch_beam(dp, nullptr, nullptr, stream);
}

extern "C" int ssasr_decode_beam_ctc(const ssasr_beam* dp, const ssasr_ctc_prefix* cp, void* stream) {
  if (!cp) return SSASR_EARG;
  return launch_beam(dp, cp, nullptr, stream);
}

extern "C" int ssasr_decode_beam_ex(const ssasr_beam* dp, const ssasr_ctc_prefix* cp, const ssasr_beam_terms* tp,
                                    void* stream) {
  if (!tp) return SSASR_EARG;
  return launch_beam(dp, cp, tp, stream);
}

extern "C" int ssasr_decode_sample(const ssasr_beam* dp, const ssasr_sample* sp, void* stream) {
  SampleDev s{};
  if (!sp || !sp->uniforms || (reinterpret_cast<uintptr_t>(sp->uniforms) & 3) != 0) return SSASR_EARG;
  if (!(std::isfinite(sp->temperature) && sp->temperature > 0.f)) return SSASR_EARG;
  const auto need = [](const ssasr_beam& d, int Hl) {
    return ssasr_decode_sample_ws_bytes(d.N, d.K, d.T, d.E, d.A, d.D, d.V, Hl, d.max_steps);
  };
  if (!beam_dev(dp, need, s.b)) return SSASR_EARG;
  s.uniforms = sp->uniforms; s.tau = sp->temperature; s.logq = sp->logq;
  hipLaunchKernelGGL(decode_sample_kernel, dim3((unsigned)dp->N), dim3(kThreads), 0, (hipStream_t)stream, s);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}

extern "C" int ssasr_charlm_step(const ssasr_charlm* lm, const int32_t* x, const float* h1, const float* h2,
                                 int64_t B, float* out, float* h1_out, float* h2_out, void* stream) {
  LmStepDev p{};
  if (!lm_ok(lm, p.lm) || !x || !h1 || !h2 || !out || !h1_out || !h2_out || B <= 0 || B > 0x7fffffff ||
      lm->V > 0x7fffffff)
    return SSASR_EARG;
  p.V = (int)lm->V; p.x = x; p.h1 = h1; p.h2 = h2; p.out = out; p.h1_out = h1_out; p.h2_out = h2_out;
  const size_t bytes = sizeof(float) * 9 * (size_t)lm->H;
  if (const int rc = allow_lds(reinterpret_cast<const void*>(charlm_step_kernel), bytes)) return rc;
  hipLaunchKernelGGL(charlm_step_kernel, dim3((unsigned)B), dim3(kThreads), bytes, (hipStream_t)stream, p);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}

namespace {

bool ctc_lm_shape_ok(int64_t B, int64_t T, int64_t V, int64_t K, int64_t H) {
  return ctc_prefix::shape_ok(B, T, V, K) && H >= 0 && H <= 4096 && H % 4 == 0;
}

// bytes of the float blocks, then of the texts; the lm_frames words follow
int64_t ctc_lm_float_bytes(int64_t B, int64_t K, int64_t H) { return B * ctc_lm_ws_map((int)K, (int)H).total * 4; }
int64_t ctc_lm_text_bytes(int64_t B, int64_t T, int64_t K) { return (B * 2 * K * T * 4 + 15) / 16 * 16; }

}  // namespace

extern "C" int64_t ssasr_ctc_decode_lm_ws_bytes(int64_t B, int64_t T, int64_t V, int64_t K, int64_t H) {
  if (!ctc_lm_shape_ok(B, T, V, K, H)) return 0;
  return ctc_lm_float_bytes(B, K, H) + ctc_lm_text_bytes(B, T, K) + B * 4;
}

extern "C" int ssasr_ctc_decode_lm(const float* logits, const int32_t* frame_lens, int64_t B, int64_t T, int64_t V,
                                   int64_t K, int blank, void* ws, int64_t ws_bytes, int32_t* chars, int32_t* n_chars,
                                   float* scores, int32_t* n_hyps, const ssasr_charlm* lm, float lm_weight,
                                   float length_bonus, int eos, float* ctc_scores, float* lm_scores, void* stream) {
  if (!logits || !frame_lens || !ws || !chars || !n_chars || !scores || !n_hyps || !ctc_scores || !lm_scores)
    return SSASR_EARG;
  if (!std::isfinite(lm_weight) || !std::isfinite(length_bonus) || eos >= V) return SSASR_EARG;
  CtcLmDev a{};
  if (lm && (!lm_ok(lm, a.lm) || lm->V != V)) return SSASR_EARG;
  if (lm_weight != 0.f && !lm) return SSASR_EARG;
  if (lm_weight == 0.f) a.lm = LmDev{};                       // weight 0: the LM is unread, no step runs
  const int64_t H = a.lm.H;
  if (!ctc_lm_shape_ok(B, T, V, K, H) || blank < 0 || blank >= V) return SSASR_EARG;
  if (!aligned16(ws) || ws_bytes < ssasr_ctc_decode_lm_ws_bytes(B, T, V, K, H)) return SSASR_EARG;
  char* base = reinterpret_cast<char*>(ws);
  a.d = ctc_prefix::make_args(logits, frame_lens, T, V, K, blank, base + ctc_lm_float_bytes(B, K, H), chars, n_chars,
                              scores, n_hyps);
  a.eos = eos < 0 ? -1 : eos;
  a.lm_weight = lm_weight; a.length_bonus = length_bonus;
  a.fws = reinterpret_cast<float*>(base);
  a.lm_frames = reinterpret_cast<int32_t*>(base + ctc_lm_float_bytes(B, K, H) + ctc_lm_text_bytes(B, T, K));
  a.ctc_scores = ctc_scores; a.lm_scores = lm_scores;
  hipLaunchKernelGGL(ctc_prefix_beam_lm_kernel, dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, a);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}
