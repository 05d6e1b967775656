// Inference: the greedy decode loop of ASR.decode (src/asr.py:112-173) with the CharLM term
// (src/charlm.py:46-57) as ONE launch for N encoded utterances, and one CharLM step for callers
// that drive the language model themselves.
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
#include <cmath>
#include "../../include/ssasr.h"
#include "common.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kRows = 4;                 // rows of a matrix-vector product a wave has in flight
constexpr size_t kMaxLds = 160 * 1024;   // LDS of one CU

__device__ __forceinline__ float dot4(const float4& a, const float4& b, float acc) {
  acc = fmaf(a.x, b.x, acc);
  acc = fmaf(a.y, b.y, acc);
  acc = fmaf(a.z, b.z, acc);
  return fmaf(a.w, b.w, acc);
}
__device__ __forceinline__ float sigmoid_exact(float x) { return 1.0f / (1.0f + expf(-x)); }

// out[r] = act(w1[r][0..k1) . x1 + w2[r][0..k2) . x2 + b1[r] + b2[r]) for r < rows; x1 / x2 in LDS,
// 16-byte aligned, k1 / k2 multiples of 4 (k2 = 0: one segment); b1 / b2 optional.  act 1 = tanh.
// Called by every wave of the workgroup; rows are dealt to waves in groups of kRows.
__device__ void matvec(const float* w1, int64_t ld1, const float* x1, int k1,
                       const float* w2, int64_t ld2, const float* x2, int k2,
                       const float* __restrict__ b1, const float* __restrict__ b2, int rows, int act, float* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r0 = wave * kRows; r0 < rows; r0 += kWaves * kRows) {
    float acc[kRows];
    const float* p1[kRows];
    const float* p2[kRows];
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      const int r = min(r0 + j, rows - 1);          // rows past the end repeat the last one and are dropped
      acc[j] = 0.f;
      p1[j] = w1 + (int64_t)r * ld1;
      p2[j] = k2 ? w2 + (int64_t)r * ld2 : nullptr;
    }
    for (int k = lane * 4; k < k1; k += 256) {
      const float4 x = *reinterpret_cast<const float4*>(x1 + k);
#pragma unroll
      for (int j = 0; j < kRows; ++j) acc[j] = dot4(*reinterpret_cast<const float4*>(p1[j] + k), x, acc[j]);
    }
    for (int k = lane * 4; k < k2; k += 256) {
      const float4 x = *reinterpret_cast<const float4*>(x2 + k);
#pragma unroll
      for (int j = 0; j < kRows; ++j) acc[j] = dot4(*reinterpret_cast<const float4*>(p2[j] + k), x, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < kRows; ++j) acc[j] = wave_sum(acc[j]);
    if (lane < kRows && r0 + lane < rows) {
      const int r = r0 + lane;
      float v = lane == 0 ? acc[0] : lane == 1 ? acc[1] : lane == 2 ? acc[2] : acc[3];
      if (b1) v += b1[r];
      if (b2) v += b2[r];
      out[r] = act == 1 ? tanhf(v) : v;
    }
  }
}

// nn.LSTMCell's update from the pre-activations g [4H] (order i, f, g, o; src/asr.py:320-324)
__device__ void lstm_update(const float* g, float* h, float* c, int H) {
  for (int u = threadIdx.x; u < H; u += kThreads) {
    const float i = sigmoid_exact(g[u]), f = sigmoid_exact(g[H + u]), gg = tanhf(g[2 * H + u]),
                o = sigmoid_exact(g[3 * H + u]);
    const float cn = f * c[u] + i * gg;
    c[u] = cn;
    h[u] = o * tanhf(cn);
  }
}

// nn.GRUCell's update from gi = W_ih x + b_ih and gh = W_hh h + b_hh [3H] (order r, z, n)
__device__ void gru_update(const float* gi, const float* gh, float* h, int H) {
  for (int u = threadIdx.x; u < H; u += kThreads) {
    const float r = sigmoid_exact(gi[u] + gh[u]), z = sigmoid_exact(gi[H + u] + gh[H + u]);
    const float n = tanhf(gi[2 * H + u] + r * gh[2 * H + u]);
    h[u] = (1.f - z) * n + z * h[u];
  }
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

  // comp = tanh(psi(feat)) for this utterance's frames, once (src/asr.py:381): a wave takes a row of
  // W_psi against four frames at a time
  for (int a = wave; a < A; a += kWaves) {
    const float* wrow = p.w_psi + (int64_t)a * E;
    const float bias = p.b_psi[a];
    for (int t0 = 0; t0 < len; t0 += kRows) {
      float acc[kRows];
      const float* f[kRows];
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        acc[j] = 0.f;
        f[j] = feat + (int64_t)min(t0 + j, len - 1) * E;
      }
      for (int k = lane * 4; k < E; k += 256) {
        const float4 w = *reinterpret_cast<const float4*>(wrow + k);
#pragma unroll
        for (int j = 0; j < kRows; ++j) acc[j] = dot4(*reinterpret_cast<const float4*>(f[j] + k), w, acc[j]);
      }
#pragma unroll
      for (int j = 0; j < kRows; ++j) acc[j] = wave_sum(acc[j]);
      if (lane < kRows && t0 + lane < len) {
        const float v = lane == 0 ? acc[0] : lane == 1 ? acc[1] : lane == 2 ? acc[2] : acc[3];
        comp[(int64_t)(t0 + lane) * A + a] = tanhf(v + bias);
      }
    }
  }
  // zero states (src/asr.py:133-134), <SOS> = 0 as the first input character (:137-138)
  for (int i = tid; i < 4 * D; i += kThreads) lds[m.h1 + i] = 0.f;
  for (int i = tid; i < 2 * Hl; i += kThreads) lmh1[i] = 0.f;       // lmh1 and lmh2 are adjacent
  copy_row(xin, p.embed, D);
  if (Hl) copy_row(lmx, p.lm.emb, Hl);
  __syncthreads();

  const int ncol4 = E / 4;
  const int G = ncol4 >= kThreads ? 1 : kThreads / ncol4;          // frame groups of the context sum
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
    if (Hl) gru_update(gi, gh, lmh1, Hl);
    matvec(comp, A, q, A, nullptr, 0, nullptr, 0, nullptr, nullptr, len, 0, en);
    __syncthreads();
    // 3: softmax over the frames (src/asr.py:388) | LM layer 2 products (src/charlm.py:55)
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
    // 4: context = att . feat (src/asr.py:389-390): a thread sums one float4 column over its group's frames
    if (G == 1) {
      for (int c = tid; c < ncol4; c += kThreads) {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int t = 0; t < len; ++t) {
          const float4 v = *reinterpret_cast<const float4*>(feat + (int64_t)t * E + c * 4);
          const float a = en[t];
          s.x = fmaf(a, v.x, s.x); s.y = fmaf(a, v.y, s.y); s.z = fmaf(a, v.z, s.z); s.w = fmaf(a, v.w, s.w);
        }
        *reinterpret_cast<float4*>(xin + D + c * 4) = s;
      }
    } else {
      const int c = tid % ncol4, g = tid / ncol4;
      if (g < G) {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int t = g; t < len; t += G) {
          const float4 v = *reinterpret_cast<const float4*>(feat + (int64_t)t * E + c * 4);
          const float a = en[t];
          s.x = fmaf(a, v.x, s.x); s.y = fmaf(a, v.y, s.y); s.z = fmaf(a, v.z, s.z); s.w = fmaf(a, v.w, s.w);
        }
        *reinterpret_cast<float4*>(part + (g * ncol4 + c) * 4) = s;
      }
    }
    if (Hl) gru_update(gi, gh, lmh2, Hl);
    __syncthreads();
    if (G > 1) {
      for (int e = tid; e < E; e += kThreads) {
        float s = part[e];
        for (int g = 1; g < G; ++g) s += part[g * E + e];
        xin[D + e] = s;
      }
      __syncthreads();
    }
    // 5: Speller cell 1 on [embedding | context] (src/asr.py:149-150, :320-321) | LM output layer (src/charlm.py:56)
    matvec(p.w_ih1, D + E, xin, D + E, p.w_hh1, D, h1, D, p.b_ih1, p.b_hh1, 4 * D, 0, gates);
    if (Hl) matvec(p.lm.w_out, Hl, lmh2, Hl, nullptr, 0, nullptr, 0, p.lm.b_out, nullptr, V, 0, lmlg);
    __syncthreads();
    lstm_update(gates, h1, c1, D);
    __syncthreads();
    // 6: cell 2 (src/asr.py:323-324)
    matvec(p.w_ih2, D, h1, D, p.w_hh2, D, h2, D, p.b_ih2, p.b_hh2, 4 * D, 0, gates);
    __syncthreads();
    lstm_update(gates, h2, c2, D);
    __syncthreads();
    // 7: char_trans (src/asr.py:153)
    matvec(p.w_ct, D, h2, D, nullptr, 0, nullptr, 0, p.b_ct, nullptr, V, 0, lg);
    __syncthreads();
    // 8: final = log_softmax(asr) + lm_weight * log_softmax(lm), first maximum wins (src/asr.py:153-159)
    if (wave == 0) {
      const float x = lane < V ? lg[lane] : -INFINITY;
      const float xm = wave_max(x);
      const float xs = wave_sum(lane < V ? expf(x - xm) : 0.f);
      float fin = x - xm - logf(xs);
      if (Hl) {
        const float y = lane < V ? lmlg[lane] : -INFINITY;
        const float ym = wave_max(y);
        const float ys = wave_sum(lane < V ? expf(y - ym) : 0.f);
        fin = fin + p.lm_weight * (y - ym - logf(ys));
      }
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
  gru_update(gi, gh, h1, H);
  __syncthreads();
  matvec(p.lm.w_ih2, H, h1, H, nullptr, 0, nullptr, 0, p.lm.b_ih2, nullptr, 3 * H, 0, gi);
  matvec(p.lm.w_hh2, H, h2, H, nullptr, 0, nullptr, 0, p.lm.b_hh2, nullptr, 3 * H, 0, gh);
  __syncthreads();
  gru_update(gi, gh, h2, H);
  __syncthreads();
  matvec(p.lm.w_out, H, h2, H, nullptr, 0, nullptr, 0, p.lm.b_out, nullptr, p.V, 0, p.out + (int64_t)b * p.V);
  copy_row(p.h1_out + (int64_t)b * H, h1, H);
  copy_row(p.h2_out + (int64_t)b * H, h2, H);
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

}  // namespace

extern "C" int ssasr_decode_greedy(const ssasr_infer* dp, void* stream) {
  if (!dp) return SSASR_EARG;
  const ssasr_infer& d = *dp;
  // the dimensions ssasr_decoder_fwd takes, with V <= 64 (one wave holds a score row)
  if (d.N <= 0 || d.N > 0x7fffffff || d.T <= 0 || d.T > 16384 || d.E <= 0 || d.E > 8192 || d.E % 4 != 0 || d.A <= 0 ||
      d.A > 2048 || d.A % 4 != 0 || d.D <= 0 || d.D > 4096 || d.D % 16 != 0 || d.V <= 0 || d.V > 64 ||
      d.max_steps <= 0 || d.max_steps > (1 << 20) || d.eos < 0 || d.eos >= d.V)
    return SSASR_EARG;
  const void* need[] = {d.feat, d.enc_len, d.comp, d.w_psi, d.b_psi, d.w_phi, d.w_ih1, d.w_hh1, d.b_ih1, d.b_hh1,
                        d.w_ih2, d.w_hh2, d.b_ih2, d.b_hh2, d.embed, d.w_ct, d.b_ct, d.chars, d.n_chars, d.scores};
  for (const void* q : need)
    if (!q) return SSASR_EARG;
  const void* vec[] = {d.feat, d.comp, d.w_psi, d.w_phi, d.w_ih1, d.w_hh1, d.w_ih2, d.w_hh2, d.embed, d.w_ct};
  for (const void* q : vec)
    if (!aligned16(q)) return SSASR_EARG;
  InferDev p{};
  if (d.lm) {
    if (!lm_ok(d.lm, p.lm) || d.lm->V != d.V) return SSASR_EARG;
  }
  const size_t bytes = sizeof(float) * (size_t)lds_map((int)d.T, (int)d.E, (int)d.A, (int)d.D, p.lm.H).total;
  if (bytes > kMaxLds) return SSASR_EARG;
  p.T = (int)d.T; p.E = (int)d.E; p.A = (int)d.A; p.D = (int)d.D; p.V = (int)d.V;
  p.max_steps = (int)d.max_steps; p.eos = d.eos; p.lm_weight = d.lm ? d.lm_weight : 0.f;
  p.feat = d.feat; p.enc_len = d.enc_len; p.comp = d.comp; p.w_psi = d.w_psi; p.b_psi = d.b_psi; p.w_phi = d.w_phi;
  p.w_ih1 = d.w_ih1; p.w_hh1 = d.w_hh1; p.b_ih1 = d.b_ih1; p.b_hh1 = d.b_hh1;
  p.w_ih2 = d.w_ih2; p.w_hh2 = d.w_hh2; p.b_ih2 = d.b_ih2; p.b_hh2 = d.b_hh2;
  p.embed = d.embed; p.w_ct = d.w_ct; p.b_ct = d.b_ct;
  p.chars = d.chars; p.n_chars = d.n_chars; p.scores = d.scores; p.att = d.att;
  if (const int rc = allow_lds(reinterpret_cast<const void*>(decode_greedy_kernel), bytes)) return rc;
  hipLaunchKernelGGL(decode_greedy_kernel, dim3((unsigned)d.N), dim3(kThreads), bytes, (hipStream_t)stream, p);
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
