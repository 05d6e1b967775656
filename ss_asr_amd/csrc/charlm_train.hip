// Training the character language model: one chunk of CHARLMTrainer.exec (src/trainer.py:229-251) as one
// forward launch and one backward launch.
//
// The rows of a batch are independent recurrences.  A workgroup owns a tile of 16 batch rows (the M of
// v_mfma_f32_16x16x4_f32) for the whole chunk, forward and backward.  Nothing is exchanged between
// workgroups: no status words, no spins, no arena, no co-residency requirement.  Every loop is bounded by
// U, B, H or V.  A row's results depend on that row's inputs alone: an MFMA output element is a k-ordered
// fma chain over its own A row, and the softmax / loss / draw of a row are one wave's reductions over that
// row's classes -- the same bits at B = 1 as inside any batch.  Rows past B in the last tile compute on
// zeros and touch no global memory.
//
// Hidden states (forward) and their gradients (backward) stay in LDS for the whole chunk.  The fp32 weights
// do not fit a CU (W_hh1 alone is 196 KB at H = 128): every step streams them from L2, 16 bytes per lane,
// as the B operand of the MFMAs; a wave owns 16 hidden units and takes the r, z and n gate columns of those
// units, so that the GRU update happens in the accumulator registers.  The backward reads the TRANSPOSED
// weights, which the forward's prologue kernel writes into the workspace next to the layer-1 input table
// G1 = emb . W_ih1^T + b_ih1 (the input is an embedding: a row gather per step, no product).
// Arithmetic is fp32 throughout: fp32 MFMA, expf, tanhf, logf.
//
// Workspace (floats; ssasr_charlm_train_ws_floats), R = U * B rows, row t * B + b:
//   G1 [V][3H] | WT_hh1, WT_ih2, WT_hh2 [H][3H] each | WT_out [H][64] (classes >= V zero)
//   H1, H2 [U+1][B][H]      h before step t in row block t (block 0 zero)
//   S1, S2 [R][4H]          forward: r, z, n, W_hn h + b_hn;  after backward: d r_pre, d z_pre, d n_pre, r * d n_pre
//                           (d gi = columns [0, 3H), d gh = columns [0, 2H) and [3H, 4H))
//   DL [R][64]              forward: softmax;  after backward: d logits (classes >= V zero)
//   OH [R][64]              one-hot of the character fed to the step (the segment sum of d gi1 as a product)
#include <cmath>
#include "../../include/ssasr.h"
#include "common.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 16;       // batch rows of a workgroup
constexpr int kVp = 64;         // padded class count: one wave holds a score row
constexpr int kMaxH = 256;
constexpr int kPad = 20;        // LDS row padding (floats): row stride / 4 is 5 mod 16, b128 reads of 16 rows x 4 k-groups spread evenly

struct Layout {
  int64_t g1, wt_hh1, wt_ih2, wt_hh2, wt_out, h1, h2, s1, s2, dl, oh, total;
};
inline Layout layout(int64_t B, int64_t U, int64_t H, int64_t V) {
  Layout m;
  const int64_t R = U * B;
  int64_t o = 0;
  m.g1 = o; o += (V * 3 * H + 15) / 16 * 16;
  m.wt_hh1 = o; o += H * 3 * H;
  m.wt_ih2 = o; o += H * 3 * H;
  m.wt_hh2 = o; o += H * 3 * H;
  m.wt_out = o; o += H * kVp;
  m.h1 = o; o += (U + 1) * B * H;
  m.h2 = o; o += (U + 1) * B * H;
  m.s1 = o; o += R * 4 * H;
  m.s2 = o; o += R * 4 * H;
  m.dl = o; o += R * kVp;
  m.oh = o; o += R * kVp;
  m.total = o;
  return m;
}

bool shape_ok(int64_t B, int64_t U, int64_t H, int64_t V) {
  return B >= 1 && U >= 1 && V >= 1 && V <= kVp && H >= 16 && H <= kMaxH && H % 16 == 0 && B <= (1 << 24) &&
         U <= (1 << 24) && U * B <= 0x7fffffff / 4;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct TrainDev {
  int B, U, H, V;
  const float *emb, *w_ih1, *b_ih1, *w_hh1, *b_hh1, *w_ih2, *b_ih2, *w_hh2, *b_hh2, *w_out, *b_out;
  const int32_t *y, *feed, *modes;
  const float* uniforms;
  float* loss_rows;
  int32_t* fed;
  float* logits;
  float dloss;
  float *g1, *wt_hh1, *wt_ih2, *wt_hh2, *wt_out, *H1, *H2, *S1, *S2, *DL, *OH;
};

__device__ __forceinline__ float sigmoid_exact(float x) { return 1.0f / (1.0f + expf(-x)); }

// acc[g] += X[16][k0 .. k0 + 16) . W_g[16 units][k0 .. k0 + 16)^T for G matrices that share the A operand.
// xa: this lane's 4 consecutive k of its A row; w[g]: the same 4 k of its B row.  The k order inside the four
// MFMAs is (4 q + c, c = 0..3 per instruction), the same for A and B.
template <int G>
__device__ __forceinline__ void mma_k16(f32x4 (&acc)[G], const float4& xa, const float4 (&w)[G]) {
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.x, w[g].x, acc[g], 0, 0, 0);
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.y, w[g].y, acc[g], 0, 0, 0);
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.z, w[g].z, acc[g], 0, 0, 0);
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.w, w[g].w, acc[g], 0, 0, 0);
}

__device__ __forceinline__ const float4& ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// Prologue: G1 = emb . W_ih1^T + b_ih1, the transposed recurrent weights and the padded transposed output layer.
__global__ __launch_bounds__(256) void train_prologue_kernel(TrainDev p) {
  const int H = p.H, V = p.V, H3 = 3 * H;
  const int n_g1 = V * H3, n_wt = H * H3, n_out = H * kVp;
  const int total = n_g1 + 3 * n_wt + n_out;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    if (i < n_g1) {
      const int v = i / H3, j = i - v * H3;
      const float* e = p.emb + (int64_t)v * H;
      const float* w = p.w_ih1 + (int64_t)j * H;
      float acc = 0.f;
      for (int k = 0; k < H; ++k) acc = fmaf(e[k], w[k], acc);
      p.g1[i] = acc + p.b_ih1[j];
      continue;
    }
    int r = i - n_g1;
    if (r < 3 * n_wt) {
      const int which = r / n_wt;
      r -= which * n_wt;
      const int u = r / H3, c = r - u * H3;
      const float* src = which == 0 ? p.w_hh1 : which == 1 ? p.w_ih2 : p.w_hh2;
      float* dst = which == 0 ? p.wt_hh1 : which == 1 ? p.wt_ih2 : p.wt_hh2;
      dst[r] = src[(int64_t)c * H + u];
      continue;
    }
    r -= 3 * n_wt;
    const int u = r / kVp, v = r - u * kVp;
    p.wt_out[r] = v < V ? p.w_out[(int64_t)v * H + u] : 0.f;
  }
}

// nn.GRUCell from the accumulators of one 16-unit tile: gh[g][reg] is (W_hg h)[row 4 q + reg][unit], gi
// likewise (or the table row).  Writes h' to LDS and the saved activations / the new state to the workspace.
__device__ __forceinline__ float gru_unit(float gir, float giz, float gin, float ghr, float ghz, float ghn, float hold,
                                          float* save, int H, int u, bool valid) {
  const float r = sigmoid_exact(gir + ghr), z = sigmoid_exact(giz + ghz);
  const float n = tanhf(gin + r * ghn);
  if (valid) {
    save[u] = r;
    save[H + u] = z;
    save[2 * H + u] = n;
    save[3 * H + u] = ghn;
  }
  return n + z * (hold - n);
}

__global__ __launch_bounds__(kThreads) void train_fwd_kernel(TrainDev p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, q = lane >> 4;
  const int B = p.B, U = p.U, H = p.H, V = p.V, H3 = 3 * H, ldh = H + kPad;
  const int b0 = blockIdx.x * kTile;
  float* h1 = lds;                          // [2][16][ldh]
  float* h2 = h1 + 2 * kTile * ldh;         // [2][16][ldh]
  float* lg = h2 + 2 * kTile * ldh;         // [16][64]
  int* fedL = reinterpret_cast<int*>(lg + kTile * kVp);   // [16]

  for (int i = tid; i < 4 * kTile * ldh; i += kThreads) lds[i] = 0.f;
  if (tid < kTile) fedL[tid] = 0;
  for (int i = tid; i < kTile * H; i += kThreads) {
    const int row = i / H, u = i - row * H;
    if (b0 + row < B) {
      p.H1[(int64_t)(b0 + row) * H + u] = 0.f;
      p.H2[(int64_t)(b0 + row) * H + u] = 0.f;
    }
  }
  if (tid < kTile && b0 + tid < B) p.fed[b0 + tid] = 0;        // <SOS>, src/trainer.py:231
  __syncthreads();

  float loss[2] = {0.f, 0.f};               // rows 2 wave, 2 wave + 1 (lane-uniform)
  for (int t = 0; t < U; ++t) {
    const int cur = t & 1;
    const float *h1c = h1 + cur * kTile * ldh, *h2c = h2 + cur * kTile * ldh;
    float *h1n = h1 + (cur ^ 1) * kTile * ldh, *h2n = h2 + (cur ^ 1) * kTile * ldh;

    // A: layer 1.  gh1 = h1 . W_hh1^T; gi1 is the table row of the fed character (src/charlm.py:53-54)
    for (int ut = wave; ut < H / 16; ut += kWaves) {
      const int u = ut * 16 + c;
      f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      const float* w = p.w_hh1 + (int64_t)u * H + 4 * q;
      const float* x = h1c + c * ldh + 4 * q;
#pragma unroll 2
      for (int k = 0; k < H; k += 16) {
        const float4 wv[3] = {ld4(w + k), ld4(w + (int64_t)H * H + k), ld4(w + (int64_t)2 * H * H + k)};
        mma_k16<3>(acc, ld4(x + k), wv);
      }
      const float br = p.b_hh1[u], bz = p.b_hh1[H + u], bn = p.b_hh1[2 * H + u];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = 4 * q + reg;
        const bool valid = b0 + row < B;
        const float* gi = p.g1 + (int64_t)fedL[row] * H3;
        const int64_t rb = (int64_t)t * B + b0 + row;
        const float hn = gru_unit(gi[u], gi[H + u], gi[2 * H + u], acc[0][reg] + br, acc[1][reg] + bz, acc[2][reg] + bn,
                                  h1c[row * ldh + u], p.S1 + rb * 4 * H, H, u, valid);
        h1n[row * ldh + u] = hn;
        if (valid) p.H1[(rb + B) * H + u] = hn;
      }
    }
    __syncthreads();
    // B: layer 2 on the new h1 (src/charlm.py:55)
    for (int ut = wave; ut < H / 16; ut += kWaves) {
      const int u = ut * 16 + c;
      f32x4 ai[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      f32x4 ah[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      const float* wi = p.w_ih2 + (int64_t)u * H + 4 * q;
      const float* wh = p.w_hh2 + (int64_t)u * H + 4 * q;
      const float* xi = h1n + c * ldh + 4 * q;
      const float* xh = h2c + c * ldh + 4 * q;
#pragma unroll 2
      for (int k = 0; k < H; k += 16) {
        const float4 wiv[3] = {ld4(wi + k), ld4(wi + (int64_t)H * H + k), ld4(wi + (int64_t)2 * H * H + k)};
        const float4 whv[3] = {ld4(wh + k), ld4(wh + (int64_t)H * H + k), ld4(wh + (int64_t)2 * H * H + k)};
        mma_k16<3>(ai, ld4(xi + k), wiv);
        mma_k16<3>(ah, ld4(xh + k), whv);
      }
      const float bir = p.b_ih2[u], biz = p.b_ih2[H + u], bin = p.b_ih2[2 * H + u];
      const float bhr = p.b_hh2[u], bhz = p.b_hh2[H + u], bhn = p.b_hh2[2 * H + u];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = 4 * q + reg;
        const bool valid = b0 + row < B;
        const int64_t rb = (int64_t)t * B + b0 + row;
        const float hn = gru_unit(ai[0][reg] + bir, ai[1][reg] + biz, ai[2][reg] + bin, ah[0][reg] + bhr, ah[1][reg] + bhz,
                                  ah[2][reg] + bhn, h2c[row * ldh + u], p.S2 + rb * 4 * H, H, u, valid);
        h2n[row * ldh + u] = hn;
        if (valid) p.H2[(rb + B) * H + u] = hn;
      }
    }
    __syncthreads();
    // C: the output layer (src/charlm.py:56)
    for (int vt = wave; vt * 16 < V; vt += kWaves) {
      const int v = vt * 16 + c, vr = min(v, V - 1);      // classes past V repeat the last row and are dropped
      f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      const float* w = p.w_out + (int64_t)vr * H + 4 * q;
      const float* x = h2n + c * ldh + 4 * q;
      for (int k = 0; k < H; k += 16) {
        const float4 wv = ld4(w + k), xv = ld4(x + k);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.x, wv.x, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.y, wv.y, acc[1], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.z, wv.z, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.w, wv.w, acc[1], 0, 0, 0);
      }
      const float bo = p.b_out[vr];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) lg[(4 * q + reg) * kVp + v] = acc[0][reg] + acc[1][reg] + bo;
    }
    __syncthreads();
    // D: log-softmax, -log p[y] (src/trainer.py:238-239), the next character (:241-246); a wave per row
    const int mode = p.modes[t];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const int row = 2 * wave + rr, b = b0 + row;
      const bool valid = b < B;
      const float x = lane < V ? lg[row * kVp + lane] : -INFINITY;
      const float mx = wave_max(x);
      const float e = lane < V ? expf(x - mx) : 0.f;
      const float s = wave_sum(e);
      const int yb = valid ? min(max(p.y[(int64_t)b * U + t], 0), V - 1) : 0;
      const float xy = __shfl(x, yb, 64);
      loss[rr] += -(xy - mx - logf(s));
      int nx = valid ? min(max(p.feed[(int64_t)b * U + t], 0), V - 1) : 0;
      if (mode == 1 && p.uniforms) {
        // first v with cumsum(softmax)[v] > u * total (Categorical.sample for a caller-supplied uniform)
        float run = e;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const float up = __shfl_up(run, off, 64);
          if (lane >= off) run += up;
        }
        const float tot = __shfl(run, 63, 64);
        const float target = (valid ? p.uniforms[(int64_t)t * B + b] : 0.f) * tot;
        const unsigned long long over = __ballot(lane < V && run > target);
        nx = over ? __builtin_ctzll(over) : V - 1;
      }
      const int was = fedL[row];
      if (valid) {
        const int64_t rb = (int64_t)t * B + b;
        p.DL[rb * kVp + lane] = e / s;
        p.OH[rb * kVp + lane] = lane == was ? 1.f : 0.f;
        if (p.logits && lane < V) p.logits[rb * V + lane] = x;
        if (lane == 0) p.fed[rb + B] = nx;
      }
      if (lane == 0) fedL[row] = nx;       // only this wave reads or writes fedL[row] in this phase
    }
    __syncthreads();
  }
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    const int b = b0 + 2 * wave + rr;
    if (lane == 0 && b < B) p.loss_rows[b] = loss[rr];
  }
}

// d of one GRU unit from d h' (dh): the saved r, z, n, gh_n become d r_pre, d z_pre, d n_pre, r * d n_pre in the
// workspace (valid rows) and in the LDS image; returns the direct part of d h, dh * z.
__device__ __forceinline__ float gru_unit_bwd(float dh, float hprev, float* save, float* dg, int H, int u, bool valid) {
  float r = 0.f, z = 0.f, n = 0.f, ghn = 0.f;
  if (valid) {
    r = save[u];
    z = save[H + u];
    n = save[2 * H + u];
    ghn = save[3 * H + u];
  }
  const float dn_pre = dh * (1.f - z) * (1.f - n * n);
  const float dz_pre = dh * (hprev - n) * z * (1.f - z);
  const float dr_pre = dn_pre * ghn * r * (1.f - r);
  const float rdn = r * dn_pre;
  if (valid) {
    save[u] = dr_pre;
    save[H + u] = dz_pre;
    save[2 * H + u] = dn_pre;
    save[3 * H + u] = rdn;
  }
  dg[u] = dr_pre;
  dg[H + u] = dz_pre;
  dg[2 * H + u] = dn_pre;
  dg[3 * H + u] = rdn;
  return dh * z;
}

__global__ __launch_bounds__(kThreads) void train_bwd_kernel(TrainDev p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, q = lane >> 4;
  const int B = p.B, U = p.U, H = p.H, V = p.V, H3 = 3 * H, ldh = H + kPad, ldg = 4 * H + kPad, ldl = kVp + kPad;
  const int b0 = blockIdx.x * kTile;
  float* dh1 = lds;                      // [16][ldh]  d loss / d h1 after step t, from the steps behind it
  float* dh2 = dh1 + kTile * ldh;        // [16][ldh]
  float* dg = dh2 + kTile * ldh;         // [16][ldg]  the derivatives of the layer in hand
  float* dl = dg + kTile * ldg;          // [16][ldl]  d logits
  for (int i = tid; i < 2 * kTile * ldh; i += kThreads) lds[i] = 0.f;
  __syncthreads();

  for (int t = U - 1; t >= 0; --t) {
    // 1: d logits = (softmax - onehot(y)) * d loss_row, in place
    for (int i = tid; i < kTile * kVp; i += kThreads) {
      const int row = i >> 6, v = i & 63, b = b0 + row;
      float d = 0.f;
      if (b < B) {
        const int64_t rb = (int64_t)t * B + b;
        if (v < V) {
          const int yb = min(max(p.y[(int64_t)b * U + t], 0), V - 1);
          d = (p.DL[rb * kVp + v] - (v == yb ? 1.f : 0.f)) * p.dloss;
        }
        p.DL[rb * kVp + v] = d;
      }
      dl[row * ldl + v] = d;
    }
    __syncthreads();
    // 2: d h2' = carry + d logits . W_out, then layer 2's gate derivatives
    for (int ut = wave; ut < H / 16; ut += kWaves) {
      const int u = ut * 16 + c;
      f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      const float* w = p.wt_out + (int64_t)u * kVp + 4 * q;
      const float* x = dl + c * ldl + 4 * q;
#pragma unroll
      for (int k = 0; k < kVp; k += 16) {
        const float4 wv = ld4(w + k), xv = ld4(x + k);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.x, wv.x, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.y, wv.y, acc[1], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.z, wv.z, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.w, wv.w, acc[1], 0, 0, 0);
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = 4 * q + reg;
        const bool valid = b0 + row < B;
        const int64_t rb = (int64_t)t * B + b0 + row;
        const float dh = dh2[row * ldh + u] + (acc[0][reg] + acc[1][reg]);
        const float hprev = valid ? p.H2[rb * H + u] : 0.f;
        dh2[row * ldh + u] = gru_unit_bwd(dh, hprev, p.S2 + rb * 4 * H, dg + row * ldg, H, u, valid);
      }
    }
    __syncthreads();
    // 3: d h2 += d gh2 . W_hh2 (into the carry), d h1' += d gi2 . W_ih2
    for (int ut = wave; ut < H / 16; ut += kWaves) {
      const int u = ut * 16 + c;
      f32x4 ah[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      f32x4 ai[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      const float* wh = p.wt_hh2 + (int64_t)u * H3 + 4 * q;
      const float* wi = p.wt_ih2 + (int64_t)u * H3 + 4 * q;
      const float* x = dg + c * ldg + 4 * q;
#pragma unroll 2
      for (int k = 0; k < H3; k += 16) {      // four independent chains
        const float4 xi = ld4(x + k), xh = ld4(x + (k < 2 * H ? k : k + H));
        const float4 wiv = ld4(wi + k), whv = ld4(wh + k);
        ai[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(xi.x, wiv.x, ai[0], 0, 0, 0);
        ah[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(xh.x, whv.x, ah[0], 0, 0, 0);
        ai[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(xi.y, wiv.y, ai[1], 0, 0, 0);
        ah[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(xh.y, whv.y, ah[1], 0, 0, 0);
        ai[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(xi.z, wiv.z, ai[0], 0, 0, 0);
        ah[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(xh.z, whv.z, ah[0], 0, 0, 0);
        ai[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(xi.w, wiv.w, ai[1], 0, 0, 0);
        ah[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(xh.w, whv.w, ah[1], 0, 0, 0);
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = 4 * q + reg;
        dh2[row * ldh + u] += ah[0][reg] + ah[1][reg];
        dh1[row * ldh + u] += ai[0][reg] + ai[1][reg];
      }
    }
    __syncthreads();
    // 4: layer 1's gate derivatives
    for (int ut = wave; ut < H / 16; ut += kWaves) {
      const int u = ut * 16 + c;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = 4 * q + reg;
        const bool valid = b0 + row < B;
        const int64_t rb = (int64_t)t * B + b0 + row;
        const float hprev = valid ? p.H1[rb * H + u] : 0.f;
        dh1[row * ldh + u] = gru_unit_bwd(dh1[row * ldh + u], hprev, p.S1 + rb * 4 * H, dg + row * ldg, H, u, valid);
      }
    }
    __syncthreads();
    // 5: d h1 += d gh1 . W_hh1.  The next step's phase 1 touches neither dg nor dh1, and its barrier stands
    // between these reads of dg and phase 2's writes.
    for (int ut = wave; ut < H / 16; ut += kWaves) {
      const int u = ut * 16 + c;
      f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      const float* w = p.wt_hh1 + (int64_t)u * H3 + 4 * q;
      const float* x = dg + c * ldg + 4 * q;
#pragma unroll 2
      for (int k = 0; k < H3; k += 16) {
        const float4 wv = ld4(w + k), xv = ld4(x + (k < 2 * H ? k : k + H));
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.x, wv.x, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.y, wv.y, acc[1], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.z, wv.z, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.w, wv.w, acc[1], 0, 0, 0);
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) dh1[(4 * q + reg) * ldh + u] += acc[0][reg] + acc[1][reg];
    }
  }
}

bool fill(const ssasr_charlm* lm, int64_t B, int64_t U, float* ws, TrainDev& p) {
  if (!lm || !shape_ok(B, U, lm->H, lm->V) || !ws || !aligned16(ws)) return false;
  const float* ptrs[] = {lm->emb, lm->w_ih1, lm->w_hh1, lm->b_ih1, lm->b_hh1, lm->w_ih2, lm->w_hh2, lm->b_ih2,
                         lm->b_hh2, lm->w_out, lm->b_out};
  for (const float* q : ptrs)
    if (!q || !aligned16(q)) return false;
  p.B = (int)B; p.U = (int)U; p.H = (int)lm->H; p.V = (int)lm->V;
  p.emb = lm->emb; p.w_ih1 = lm->w_ih1; p.b_ih1 = lm->b_ih1; p.w_hh1 = lm->w_hh1; p.b_hh1 = lm->b_hh1;
  p.w_ih2 = lm->w_ih2; p.b_ih2 = lm->b_ih2; p.w_hh2 = lm->w_hh2; p.b_hh2 = lm->b_hh2;
  p.w_out = lm->w_out; p.b_out = lm->b_out;
  const Layout m = layout(B, U, lm->H, lm->V);
  p.g1 = ws + m.g1; p.wt_hh1 = ws + m.wt_hh1; p.wt_ih2 = ws + m.wt_ih2; p.wt_hh2 = ws + m.wt_hh2;
  p.wt_out = ws + m.wt_out; p.H1 = ws + m.h1; p.H2 = ws + m.h2; p.S1 = ws + m.s1; p.S2 = ws + m.s2;
  p.DL = ws + m.dl; p.OH = ws + m.oh;
  return true;
}

int allow_lds(const void* kernel, size_t bytes) {
  if (bytes > 64 * 1024)
    SSASR_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return SSASR_OK;
}

}  // namespace

extern "C" int64_t ssasr_charlm_train_ws_floats(int64_t B, int64_t U, int64_t H, int64_t V) {
  return shape_ok(B, U, H, V) ? layout(B, U, H, V).total : 0;
}

extern "C" int ssasr_charlm_train_fwd(const ssasr_charlm* lm, const int32_t* y, const int32_t* feed,
                                      const int32_t* modes, const float* uniforms, int64_t B, int64_t U,
                                      float* loss_rows, int32_t* fed, float* logits, float* ws, void* stream) {
  TrainDev p{};
  if (!fill(lm, B, U, ws, p) || !y || !feed || !modes || !loss_rows || !fed) return SSASR_EARG;
  p.y = y; p.feed = feed; p.modes = modes; p.uniforms = uniforms;
  p.loss_rows = loss_rows; p.fed = fed; p.logits = logits;
  const int H = p.H;
  const int pro = p.V * 3 * H + 3 * H * 3 * H + H * kVp;
  hipLaunchKernelGGL(train_prologue_kernel, dim3((unsigned)((pro + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
  SSASR_LAUNCH_CHECK();
  const size_t bytes = sizeof(float) * (size_t)(4 * kTile * (H + kPad) + kTile * kVp + kTile);
  if (const int rc = allow_lds(reinterpret_cast<const void*>(train_fwd_kernel), bytes)) return rc;
  hipLaunchKernelGGL(train_fwd_kernel, dim3((unsigned)((B + kTile - 1) / kTile)), dim3(kThreads), bytes,
                     (hipStream_t)stream, p);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}

extern "C" int ssasr_charlm_train_bwd(const ssasr_charlm* lm, const int32_t* y, int64_t B, int64_t U, float dloss,
                                      float* ws, void* stream) {
  TrainDev p{};
  if (!fill(lm, B, U, ws, p) || !y) return SSASR_EARG;
  p.y = y; p.dloss = dloss;
  const int H = p.H;
  const size_t bytes = sizeof(float) * (size_t)(2 * kTile * (H + kPad) + kTile * (4 * H + kPad) + kTile * (kVp + kPad));
  if (const int rc = allow_lds(reinterpret_cast<const void*>(train_bwd_kernel), bytes)) return rc;
  hipLaunchKernelGGL(train_bwd_kernel, dim3((unsigned)((B + kTile - 1) / kTile)), dim3(kThreads), bytes,
                     (hipStream_t)stream, p);
  SSASR_LAUNCH_CHECK();
  return SSASR_OK;
}
