// Content-based attention of the Speller (reference: Attention.forward,
// src/asr.py:343-392) for one decode step:
//
//   q      = tanh(phi(s))                      [B, A]
//   e[b,t] = comp[b,t,:] . q[b,:]              comp = tanh(psi(h)), cached
//   e[b,t] = -inf for t >= enc_len[b]
//   alpha  = softmax_t(e)                      [B, T]
//   ctx[b] = sum_t alpha[b,t] * h[b,t,:]       [B, E]
//
// The step streams comp (B*T*A) and h (B*T*E) once: it is bandwidth bound
// (8.19 MB per call at B=32, T=100, A=128, E=512, fp32).  One
// workgroup handles one utterance and one slice of the E feature columns, so
// the grid is B x nch workgroups; every workgroup re-derives q and the
// softmax of its utterance (comp is small next to h) and no inter-workgroup
// exchange is needed.  All global reads are 16-byte per lane and contiguous
// per half-wave; reductions are wave shuffles plus one LDS hop.  The phi
// projection q = tanh(W_phi s) runs as its own small MFMA launch
// (seg_matmul_plain_kernel with a tanh epilogue): inside this kernel it would
// re-read the 128 KB weight per workgroup, more than the step's real payload.
#pragma once
#include "common.h"

namespace {

struct AttnFwd {
  const float* q;        // [B][A] tanh(phi(state)) from the phi kernel; null => zeros (step 0)
  const float* comp;     // [B][T][A]
  const float* feat;     // [B][T][E]
  const int32_t* lens;   // [B]
  float* att;            // out: att[b * att_sb + t]
  int64_t att_sb;
  float* ctx;            // out: ctx[b * ctx_ld + e]
  int64_t ctx_ld;
  int B, T, A, E, nch;
};

__device__ __forceinline__ float block_reduce_sum(float v, float* sm, int nw) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[w] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < nw; ++i) t += sm[i];
  return t;
}
__device__ __forceinline__ float block_reduce_max(float v, float* sm, int nw) {
  v = wave_max(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[w] = v;
  __syncthreads();
  float t = -INFINITY;
  for (int i = 0; i < nw; ++i) t = fmaxf(t, sm[i]);
  return t;
}

__device__ __forceinline__ float4 aload4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// Copies nquad float4 from global `src` to LDS `dst`, the block's threads striding by NT, EIGHT
// loads in flight per thread before the first LDS store: a plain `for (i = tid; ...) dst[i] = src[i]`
// is compiled to load -> wait -> store per iteration, i.e. one memory round trip per 4 KB of a
// 100 KB slice (~40 us at the start of a persistent decode launch).
template <int NT>
__device__ __forceinline__ void lds_fill_quads(float* dst, const float* src, int nquad, int tid) {
  int i = tid;
  for (; i + 7 * NT < nquad; i += 8 * NT) {
    float4 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = aload4(src + 4 * (int64_t)(i + k * NT));
#pragma unroll
    for (int k = 0; k < 8; ++k) *reinterpret_cast<float4*>(dst + 4 * (i + k * NT)) = v[k];
  }
  for (; i < nquad; i += NT) *reinterpret_cast<float4*>(dst + 4 * i) = aload4(src + 4 * (int64_t)i);
}

// Fast path: A == 128, E / nch == 128, T <= 128 * NP.  grid (B, nch), 256
// threads = 8 half-waves; half-wave hw owns rows t = hw + 8 i.  A lane holds 4
// of the 128 columns of its rows of comp AND of this workgroup's feat slice.
// Rows are handled in NP passes of 16 per half-wave; for NP == 1 (T <= 128,
// the training shapes) every global load of the step is issued before any
// arithmetic, i.e. one memory round trip.  The masked softmax needs one
// barrier (per-half-wave max / sum pairs combined by every thread), the
// context one more.  Workgroups of one utterance differ by a multiple of 8 in
// linear block id, so they tend to share an XCD (and its L2 copy of comp);
// nothing depends on that.
template <int NP>
__global__ __launch_bounds__(256) void attn_step_fwd_fast_kernel(AttnFwd p) {
  constexpr int RPT = 16;
  __shared__ __attribute__((aligned(16))) float sRed[8 * 128];
  __shared__ float sM[8], sS[8];
  const int b = blockIdx.x, chunk = blockIdx.y;
  const int tid = threadIdx.x, hw = tid >> 5, l32 = tid & 31;
  const int T = p.T, E = p.E;
  int len = p.lens ? p.lens[b] : T;
  len = len < T ? len : T;
  const float* cb = p.comp + (int64_t)b * T * 128 + 4 * l32;
  const float* fb = p.feat + (int64_t)b * T * E + chunk * 128 + 4 * l32;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 c[RPT], f[RPT];
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    const int t = hw + 8 * i;
    c[i] = t < len ? aload4(cb + (int64_t)t * 128) : z4;
  }
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    const int t = hw + 8 * i;
    f[i] = t < len ? aload4(fb + (int64_t)t * E) : z4;
  }
  const float4 q4 = p.q ? aload4(p.q + (int64_t)b * 128 + 4 * l32) : z4;

  // energies: dot over the 32 lanes of the half-wave
  float e[RPT * NP];
  float m = -INFINITY;
#pragma unroll
  for (int pz = 0; pz < NP; ++pz) {
    if (pz > 0) {
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        const int t = hw + 8 * (i + RPT * pz);
        c[i] = t < len ? aload4(cb + (int64_t)t * 128) : z4;
      }
    }
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      float v = c[i].x * q4.x;
      v = fmaf(c[i].y, q4.y, v);
      v = fmaf(c[i].z, q4.z, v);
      v = fmaf(c[i].w, q4.w, v);
      v = half_sum(v);
      e[pz * RPT + i] = v;
      if (hw + 8 * (i + RPT * pz) < len) m = fmaxf(m, v);
    }
  }
  float ssum = 0.f;
#pragma unroll
  for (int i = 0; i < RPT * NP; ++i) {
    const float pv = (hw + 8 * i < len) ? __builtin_amdgcn_exp2f((e[i] - m) * 1.4426950408889634f) : 0.f;
    e[i] = pv;
    ssum += pv;
  }
  if (l32 == 0) { sM[hw] = m; sS[hw] = ssum; }
  __syncthreads();
  float gm = sM[0];
#pragma unroll
  for (int g = 1; g < 8; ++g) gm = fmaxf(gm, sM[g]);
  float gs = 0.f;
#pragma unroll
  for (int g = 0; g < 8; ++g)
    gs += sS[g] > 0.f ? sS[g] * __builtin_amdgcn_exp2f((sM[g] - gm) * 1.4426950408889634f) : 0.f;
  // this half-wave's rescale: exp(m - gm) / gs   (m = -inf only when it owns no valid row)
  const float scale = ssum > 0.f
      ? __builtin_amdgcn_exp2f((m - gm) * 1.4426950408889634f) * __builtin_amdgcn_rcpf(gs) : 0.f;

  float4 acc = z4;
#pragma unroll
  for (int pz = 0; pz < NP; ++pz) {
    if (pz > 0) {
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        const int t = hw + 8 * (i + RPT * pz);
        f[i] = t < len ? aload4(fb + (int64_t)t * E) : z4;
      }
    }
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const float w = e[pz * RPT + i] * scale;
      e[pz * RPT + i] = w;
      acc.x = fmaf(w, f[i].x, acc.x);
      acc.y = fmaf(w, f[i].y, acc.y);
      acc.z = fmaf(w, f[i].z, acc.z);
      acc.w = fmaf(w, f[i].w, acc.w);
    }
  }
  if (chunk == 0 && l32 == 0) {
#pragma unroll
    for (int i = 0; i < RPT * NP; ++i) {
      const int t = hw + 8 * i;
      if (t < T) p.att[(int64_t)b * p.att_sb + t] = e[i];
    }
  }
  *reinterpret_cast<float4*>(sRed + hw * 128 + 4 * l32) = acc;
  __syncthreads();
  if (tid < 128) {
    float v = sRed[tid];
#pragma unroll
    for (int g = 1; g < 8; ++g) v += sRed[g * 128 + tid];
    p.ctx[(int64_t)b * p.ctx_ld + chunk * 128 + tid] = v;
  }
}

// Long encoder outputs (T > 256) with the same lane mapping: rows go through
// in runtime passes of 128 with the energies / alphas parked in LDS, which
// keeps the kernel below 256 VGPRs.  (Fully unrolled register variants for
// NP >= 3 make hipcc spill into AGPRs, and those builds returned wrong
// alphas on gfx950 / ROCm 7.2; see DESIGN.md.)
// grid (B, nch), 256 threads, dynamic LDS: T + 1024 + 16 floats
__global__ __launch_bounds__(256) void attn_step_fwd_long_kernel(AttnFwd p) {
  constexpr int RPT = 16;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sE = smem;                        // [T]
  float* sRed = sE + ((p.T + 3) & ~3);     // [1024]
  float* sW = sRed + 1024;                 // [16]
  const int b = blockIdx.x, chunk = blockIdx.y;
  const int tid = threadIdx.x, hw = tid >> 5, l32 = tid & 31;
  const int T = p.T, E = p.E;
  int len = p.lens ? p.lens[b] : T;
  len = len < T ? len : T;
  const float* cb = p.comp + (int64_t)b * T * 128 + 4 * l32;
  const float* fb = p.feat + (int64_t)b * T * E + chunk * 128 + 4 * l32;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 q4 = p.q ? aload4(p.q + (int64_t)b * 128 + 4 * l32) : z4;
#pragma unroll 1
  for (int t0 = 0; t0 < len; t0 += 8 * RPT) {
    float4 c[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int t = t0 + hw + 8 * i;
      c[i] = t < len ? aload4(cb + (int64_t)t * 128) : z4;
    }
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      float v = c[i].x * q4.x;
      v = fmaf(c[i].y, q4.y, v);
      v = fmaf(c[i].z, q4.z, v);
      v = fmaf(c[i].w, q4.w, v);
      v = half_sum(v);
      const int t = t0 + hw + 8 * i;
      if (l32 == 0 && t < len) sE[t] = v;
    }
  }
  __syncthreads();
  float m = -INFINITY;
  for (int t = tid; t < len; t += 256) m = fmaxf(m, sE[t]);
  m = block_reduce_max(m, sW, 4);
  float sum = 0.f;
  for (int t = tid; t < len; t += 256) {
    const float ev = __builtin_amdgcn_exp2f((sE[t] - m) * 1.4426950408889634f);
    sE[t] = ev;
    sum += ev;
  }
  sum = block_reduce_sum(sum, sW, 4);
  const float inv = sum > 0.f ? __builtin_amdgcn_rcpf(sum) : 0.f;
  for (int t = tid; t < len; t += 256) sE[t] *= inv;
  __syncthreads();
  if (chunk == 0)
    for (int t = tid; t < T; t += 256) p.att[(int64_t)b * p.att_sb + t] = t < len ? sE[t] : 0.f;

  float4 acc = z4;
#pragma unroll 1
  for (int t0 = 0; t0 < len; t0 += 8 * RPT) {
    float4 f[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int t = t0 + hw + 8 * i;
      f[i] = t < len ? aload4(fb + (int64_t)t * E) : z4;
    }
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int t = t0 + hw + 8 * i;
      const float w = t < len ? sE[t] : 0.f;
      acc.x = fmaf(w, f[i].x, acc.x);
      acc.y = fmaf(w, f[i].y, acc.y);
      acc.z = fmaf(w, f[i].z, acc.z);
      acc.w = fmaf(w, f[i].w, acc.w);
    }
  }
  *reinterpret_cast<float4*>(sRed + hw * 128 + 4 * l32) = acc;
  __syncthreads();
  if (tid < 128) {
    float v = sRed[tid];
#pragma unroll
    for (int g = 1; g < 8; ++g) v += sRed[g * 128 + tid];
    p.ctx[(int64_t)b * p.ctx_ld + chunk * 128 + tid] = v;
  }
}

// ------------------------------ split-T form ------------------------------
// Long encoder outputs (T > 128: BASELINE.json configs[3], T' up to 375) at A = 128, E = 512.
// The forms above give one utterance to E / 128 workgroups -- B x 4 = 128 of them for 256 CUs, each
// re-deriving the softmax from the whole of comp[b] -- and ran at 1.8-2.1 TB/s.  Here the FRAMES of
// an utterance are split over NS workgroups of 8 * RPH rows: every byte of comp and feat is read by
// exactly one workgroup, all of a workgroup's loads (RPH x 5 16-byte loads per lane) are in flight
// before any arithmetic, and B x NS >= 256 workgroups fill the chip.  A workgroup produces a
// partial softmax of its rows -- its own maximum m_s, S_s = sum exp(e - m_s) and the unnormalised
// partial context sum exp(e - m_s) h_t -- publishes it, and then takes part in the combination
//   M = max m_s,  S = sum_s exp(m_s - M) S_s,  ctx = sum_s exp(m_s - M) ctx_s / S,  alpha_t = exp(e_t - M) / S
// (fixed order: deterministic): workgroup s gathers the (m, S) pairs of all NS records and, of their
// partial contexts, only the column quads s, s + NS, ... (2 KB in all), writes those quads of ctx
// and the alphas of its own rows.
// Hand-off: the self-verifying exchange of the persistent recurrences (rnn_kernels.h).  Records are
// stored write-through (sc1, 16-byte stores) into a buffer that holds the NaN pattern 0x7FC0DEAD;
// readers use sc1 loads and re-fetch any 16-byte piece that still holds the pattern.  The workspace
// is TWO such buffers: a call exchanges through buffer `phase` and, first thing, restores the
// pattern in the other one (idle in this call: its last readers belong to the previous call), so
// callers alternate `phase` between consecutive calls on one workspace.
// What was measured on the way (B = 32, T' = 375, HIP-graph replay, kernel + boundary): streaming
// and publishing alone 4.9 us (6.3 TB/s); ONE workgroup per utterance combining 11-12.8 us in every
// form tried -- after a drain + returning atomic on an arrival counter, after a sentinel wait, or
// with no wait at all: its 35 KB of sc1 loads alone cost 6 us (MI355X_MICROARCH.md,
// handoff-payload: 12-20 GB/s per consumer at these sizes); a second launch for the combination
// 10.9 us (any dependent launch with a load -> compute -> store chain costs 4.8 us here).
// Every workgroup of an utterance waits for the other NS - 1: the host takes this form only when
// the occupancy query says the whole grid is resident at once; spins are bounded.
#ifndef SSASR_ATTN_VARIANT
#define SSASR_ATTN_VARIANT 0
#endif
constexpr int ATTN_PART = 512 + 32;        // floats per record: partial context (16 lines), then one line (m_s, S_s, -, ...)
#if SSASR_ATTN_VARIANT == 7                // diagnostic build: per-workgroup phase stamps (100 MHz clock)
__device__ unsigned long long g_attn_trace[8192 * 8];
#define ATTN_STAMP(k) do { if (threadIdx.x == 0) g_attn_trace[(blockIdx.y * gridDim.x + blockIdx.x) * 8 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define ATTN_STAMP(k)
#endif
constexpr unsigned ATTN_SENTINEL = 0x7FC0DEADu;

struct AttnSplit {
  const float* q;        // [B][128] or null (zeros)
  const float* comp;     // [B][T][128]
  const float* feat;     // [B][T][512]
  const int32_t* lens;   // [B] or null
  float* att;            // att[b * att_sb + t]
  int64_t att_sb;
  float* ctx;            // ctx[b * ctx_ld + e]
  int64_t ctx_ld;
  float* part;           // [2][B][NS][ATTN_PART] records; buffer `phase` is this call's
  int* status;           // one word, zero unless a hand-off of this (or an earlier) launch timed out
  int B, T, NS, phase;
  int drop_slice;        // fault injection for tests (SSASR_TEST_DROP_TILE, -1 = off): slice `drop_slice`
                         // of utterance 0 never publishes its record
};

// Bounded wait of the split kernel's gather (cf. persist_give_up, rnn_kernels.h): the first wave that
// gives up records kernel 6 + its workgroup in the status word; every other wave looks at that word
// on its 8th retry and every 256th after it, so a launch with a missing producer drains quickly.
constexpr int ATTN_PK_SPLIT = 6;
__device__ __forceinline__ bool attn_give_up(unsigned tries, unsigned max_tries, int* status) {
  if (tries > max_tries) {
    if ((threadIdx.x & 63) == 0) {
      const unsigned wg = blockIdx.x + gridDim.x * blockIdx.y;
      atomicCAS(status, 0, (int)(0x40000000u | ((unsigned)ATTN_PK_SPLIT << 24) | ((wg & 0xfffu) << 12) | 0xfffu));
    }
    return true;
  }
  return (tries & 255u) == 8u && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
}

typedef unsigned attn_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ attn_u32x4 attn_ld_raw(const __amdgpu_buffer_rsrc_t& rs, unsigned off) {
  return __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 16);        // sc1
}
__device__ __forceinline__ void attn_st_sc1(const __amdgpu_buffer_rsrc_t& rs, unsigned off, float4 v) {
  const f32x4 f = {v.x, v.y, v.z, v.w};
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(attn_u32x4, f), rs, (int)off, 0, 16);
}
__device__ __forceinline__ bool attn_unset(const attn_u32x4& v) {
  return v.x == ATTN_SENTINEL || v.y == ATTN_SENTINEL || v.z == ATTN_SENTINEL || v.w == ATTN_SENTINEL;
}
__device__ __forceinline__ float4 attn_f4(const attn_u32x4& v) {
  const f32x4 f = __builtin_bit_cast(f32x4, v);
  return make_float4(f[0], f[1], f[2], f[3]);
}

// grid (NS, B), 256 threads = 8 half-waves; half-wave hw owns rows t0 + hw + 8 i, i < RPH.  NS <= 64.
template <int RPH>
__global__ __launch_bounds__(256) void attn_step_fwd_split_kernel(AttnSplit p) {
  constexpr int R = 8 * RPH;
  constexpr float LOG2E = 1.4426950408889634f;
  constexpr unsigned MAX_TRIES = 1u << 18;
  __shared__ __attribute__((aligned(16))) float sRed[8 * 512];
  __shared__ __attribute__((aligned(16))) float sW[R];
  __shared__ float sM[8], sS[8];
  const int s = blockIdx.x, b = blockIdx.y, NS = p.NS;
  const int tid = threadIdx.x, hw = tid >> 5, l32 = tid & 31;
  const int T = p.T;
  int len = p.lens ? p.lens[b] : T;
  len = len < T ? len : T;
  const int t0 = s * R;
  const float* cb = p.comp + ((int64_t)b * T + t0) * 128 + 4 * l32;
  const float* fb = p.feat + ((int64_t)b * T + t0) * 512 + 4 * l32;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  // (requesting rows up to T instead of waiting for the utterance's length first was tried: no gain --
  // the workgroups' requests queue behind each other for ~3 us anyway -- and padded rows cost bandwidth)
  float4 c[RPH], f[RPH][4];
  const int lim = len;
#pragma unroll
  for (int i = 0; i < RPH; ++i) {
    const int r = hw + 8 * i;
    c[i] = t0 + r < lim ? aload4(cb + (int64_t)r * 128) : z4;
  }
#pragma unroll
  for (int i = 0; i < RPH; ++i) {
    const int r = hw + 8 * i;
#pragma unroll
    for (int k = 0; k < 4; ++k) f[i][k] = t0 + r < lim ? aload4(fb + (int64_t)r * 512 + 128 * k) : z4;
  }
  const float4 q4 = p.q ? aload4(p.q + (int64_t)b * 128 + 4 * l32) : z4;
  ATTN_STAMP(0);

  // the other buffer's record of this workgroup goes back to the fill pattern (nobody reads it in
  // this call); fire and forget, behind the operand loads
  const size_t buf_bytes = (size_t)p.B * NS * ATTN_PART * sizeof(float);
  const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(
      p.part + ((int64_t)(p.phase & 1) * p.B + b) * NS * ATTN_PART, 0, (int)(NS * ATTN_PART * sizeof(float)), 0x00020000);
  {
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
        p.part + ((int64_t)((p.phase & 1) ^ 1) * p.B + b) * NS * ATTN_PART, 0, (int)(NS * ATTN_PART * sizeof(float)), 0x00020000);
    const float4 fill = attn_f4(attn_u32x4{ATTN_SENTINEL, ATTN_SENTINEL, ATTN_SENTINEL, ATTN_SENTINEL});
    if (tid < ATTN_PART / 4) attn_st_sc1(ro, (unsigned)((s * ATTN_PART + 4 * tid) * 4), fill);
  }
  (void)buf_bytes;

  float e[RPH];
#pragma unroll
  for (int i = 0; i < RPH; ++i) {
    float v = c[i].x * q4.x;
    v = fmaf(c[i].y, q4.y, v);
    v = fmaf(c[i].z, q4.z, v);
    e[i] = fmaf(c[i].w, q4.w, v);
  }
#pragma unroll
  for (int i = 0; i < RPH; ++i) e[i] = half_sum(e[i]);      // independent DPP chains: the compiler interleaves them
  if (l32 == 0) {         // raw energies of this workgroup's rows, for its alphas at the end
#pragma unroll
    for (int i = 0; i < RPH; ++i) sW[hw + 8 * i] = e[i];
  }
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < RPH; ++i)
    if (t0 + hw + 8 * i < len) m = fmaxf(m, e[i]);
  if (l32 == 0) sM[hw] = m;
  __syncthreads();
  float gm = sM[0];
#pragma unroll
  for (int g = 1; g < 8; ++g) gm = fmaxf(gm, sM[g]);
  // weights relative to this workgroup's maximum, one exponential each
  float ssum = 0.f;
  float4 acc[4] = {z4, z4, z4, z4};
#pragma unroll
  for (int i = 0; i < RPH; ++i) {
    const float w = (t0 + hw + 8 * i < len) ? __builtin_amdgcn_exp2f((e[i] - gm) * LOG2E) : 0.f;
    ssum += w;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      acc[k].x = fmaf(w, f[i][k].x, acc[k].x);
      acc[k].y = fmaf(w, f[i][k].y, acc[k].y);
      acc[k].z = fmaf(w, f[i][k].z, acc[k].z);
      acc[k].w = fmaf(w, f[i][k].w, acc[k].w);
    }
  }
  if (l32 == 0) sS[hw] = ssum;
#pragma unroll
  for (int k = 0; k < 4; ++k) *reinterpret_cast<float4*>(sRed + hw * 512 + 128 * k + 4 * l32) = acc[k];
  __syncthreads();
  ATTN_STAMP(1);

  // publish this workgroup's record, write-through
  const unsigned rec = (unsigned)(s * ATTN_PART * 4);
  if (b == 0 && s == p.drop_slice) {
    // fault injection: this record stays unpublished
  } else if (tid < 128) {     // waves 0, 1: the 2 KB partial context
    float4 v = *reinterpret_cast<const float4*>(sRed + 4 * tid);
#pragma unroll
    for (int g = 1; g < 8; ++g) {
      const float4 a = *reinterpret_cast<const float4*>(sRed + g * 512 + 4 * tid);
      v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
    }
    attn_st_sc1(rp, rec + 16 * tid, v);
  } else if (tid < 136) {     // wave 2: the line of (m_s, S_s); a slice with no valid row says (0, 0), never -inf
    float gs = 0.f;
#pragma unroll
    for (int g = 0; g < 8; ++g) gs += sS[g];
    attn_st_sc1(rp, rec + 512 * 4 + 16 * (tid - 128), tid == 128 ? make_float4(gs > 0.f ? gm : 0.f, gs, 0.f, 0.f) : z4);
  }
  ATTN_STAMP(2);
#if SSASR_ATTN_VARIANT == 6       // (timing experiment: streaming and publishing only)
  return;
#endif

  // -------- gather: all pairs, and column quads s, s + NS, ... of every record's context --------
  const int QW = (128 + NS - 1) / NS;         // quads this workgroup owns (the last may not exist)
  const int L = NS * QW;                      // <= 128 + NS <= 192 pieces: thread x < L takes (record x / QW, quad x % QW)
  const int gj = tid / QW, gi = tid - gj * QW;
  const int quad = s + NS * gi;
  const bool piece = tid < L && quad < 128;
  const bool pair = tid >= 192 && tid - 192 < NS;
  const unsigned goff = piece ? (unsigned)((gj * ATTN_PART + 4 * quad) * 4)
                              : (unsigned)(((tid - 192) * ATTN_PART + 512) * 4);
  const bool want = piece || pair;
  attn_u32x4 raw = want ? attn_ld_raw(rp, goff) : attn_u32x4{0u, 0u, 0u, 0u};
  for (unsigned tries = 0; __any(want && attn_unset(raw)); ++tries) {
    if (attn_give_up(tries, MAX_TRIES, p.status)) break;      // reported: the host raises (ops.check_persistent_status)
    __builtin_amdgcn_s_sleep(2);
    if (want && attn_unset(raw)) raw = attn_ld_raw(rp, goff);
  }
  ATTN_STAMP(3);
  // Wave 3 holds the pairs, one per lane: M, S and every record's factor exp(m_j - M) / S by wave
  // shuffles (a serial loop over the NS pairs in LDS cost 4 us here: latency-bound LDS reads and
  // exponentials in every thread).
  __shared__ float sF[64], sMI[2];
  if (tid >= 192) {
    const float4 ms = pair ? attn_f4(raw) : z4;
    const bool live = pair && ms.y > 0.f;
    const float M = wave_max(live ? ms.x : -INFINITY);
    const float term = live ? ms.y * __builtin_amdgcn_exp2f((ms.x - M) * LOG2E) : 0.f;
    const float S = wave_sum(term);                      // (butterfly: every lane gets the same bits)
    const float inv = S > 0.f ? __builtin_amdgcn_rcpf(S) : 0.f;
    sF[tid - 192] = live ? __builtin_amdgcn_exp2f((ms.x - M) * LOG2E) * inv : 0.f;
    if (tid == 192) { sMI[0] = M; sMI[1] = inv; }
  }
  float* sX = sRed;                           // [NS][QW] float4 (sRed was last read before the publishing stores)
  __syncthreads();
  ATTN_STAMP(4);
  if (piece) {                                // this thread's piece, scaled by its record's factor
    const float fj = sF[gj];
    const float4 a = attn_f4(raw);
    *reinterpret_cast<float4*>(sX + 4 * tid) = make_float4(fj * a.x, fj * a.y, fj * a.z, fj * a.w);
  }
  if (tid >= 64 && tid < 64 + R) {            // the alphas of this workgroup's rows: one exponential each
    const int t = t0 + tid - 64;
    if (t < T) p.att[(int64_t)b * p.att_sb + t] = t < len ? __builtin_amdgcn_exp2f((sW[tid - 64] - sMI[0]) * LOG2E) * sMI[1] : 0.f;
  }
  __syncthreads();
  if (tid < QW && s + NS * tid < 128) {       // this workgroup's quads of ctx, records summed in order
    float4 v = z4;
#pragma unroll 8
    for (int j = 0; j < NS; ++j) {
      const float4 a = *reinterpret_cast<const float4*>(sX + 4 * (j * QW + tid));
      v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
    }
    *reinterpret_cast<float4*>(p.ctx + (int64_t)b * p.ctx_ld + 4 * (s + NS * tid)) = v;
  }
  ATTN_STAMP(5);
}

// Rows per half-wave for (B, T): the LARGEST slice that still gives every CU a workgroup (fewer
// slices = fewer records to exchange: at B = 32, T' = 375 slices of 16 / 24 / 32 / 48 rows took
// 11.8 / 9.7 / 8.8 / 8.65 us, at T' = 188 6.8 / 6.2 / 6.7 / 6.4 us -- 48 rows leave half the CUs
// idle there); when no slice size reaches 256 workgroups, the smallest (most workgroups).
inline int attn_split_rph(int B, int T) {
  if (const int forced = ssasr_options().attn_rph) return forced;
  const int sizes[4] = {6, 4, 3, 2};
  for (int rph : sizes)
    if ((int64_t)B * ((T + 8 * rph - 1) / (8 * rph)) >= 256) return rph;
  return 2;
}
inline int attn_split_ns(int B, int T) { const int R = 8 * attn_split_rph(B, T); return (T + R - 1) / R; }
// the split form is taken for T > 128 at A = 128, E = 512 when the caller provides its workspace
inline bool attn_split_ok(int64_t B, int64_t T, int64_t A, int64_t E) {
  return A == 128 && E == 512 && T > 128 && T <= 1024 && B > 0 && B <= 1024;     // NS <= 64 (sPm / sPs)
}
inline int64_t attn_split_ws_floats(int64_t B, int64_t T) {
  return 2 * B * attn_split_ns((int)B, (int)T) * (int64_t)ATTN_PART;
}

// General shapes.  grid (B, nch), 256 threads, dynamic LDS: A + T + 1024 + 16 floats
__global__ __launch_bounds__(256) void attn_step_fwd_kernel(AttnFwd p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sQ = smem;                 // [A]
  float* sE = sQ + p.A;             // [T]
  float* sR = sE + ((p.T + 3) & ~3);  // [1024]
  float* sW = sR + 1024;            // [16]
  const int b = blockIdx.x, chunk = blockIdx.y;
  const int tid = threadIdx.x;
  const int T = p.T, A = p.A, E = p.E;
  int len = p.lens ? p.lens[b] : T;
  len = len < T ? len : T;

  for (int a = tid; a < A; a += 256) sQ[a] = p.q ? p.q[(int64_t)b * A + a] : 0.f;
  __syncthreads();

  // energies: half a wave per row of comp
  {
    const int half = (tid >> 5);          // 0..7
    const int l32 = tid & 31;
    const float* cb = p.comp + (int64_t)b * T * A;
    for (int t = half; t < len; t += 8) {
      const float4* row = reinterpret_cast<const float4*>(cb + (int64_t)t * A);
      float acc = 0.f;
      for (int a4 = l32; a4 < (A >> 2); a4 += 32) {
        const float4 c = row[a4];
        const float4 qq = *reinterpret_cast<const float4*>(sQ + 4 * a4);
        acc = fmaf(c.x, qq.x, acc);
        acc = fmaf(c.y, qq.y, acc);
        acc = fmaf(c.z, qq.z, acc);
        acc = fmaf(c.w, qq.w, acc);
      }
      acc = half_sum(acc);
      if (l32 == 0) sE[t] = acc;
    }
  }
  __syncthreads();

  // masked softmax over t < len
  float m = -INFINITY;
  for (int t = tid; t < len; t += 256) m = fmaxf(m, sE[t]);
  m = block_reduce_max(m, sW, 4);
  float sum = 0.f;
  for (int t = tid; t < len; t += 256) {
    const float e = expf(sE[t] - m);
    sE[t] = e;
    sum += e;
  }
  sum = block_reduce_sum(sum, sW, 4);
  const float inv = sum > 0.f ? 1.0f / sum : 0.f;
  for (int t = tid; t < len; t += 256) sE[t] *= inv;
  __syncthreads();
  if (chunk == 0)
    for (int t = tid; t < T; t += 256) p.att[(int64_t)b * p.att_sb + t] = t < len ? sE[t] : 0.f;

  // context slice
  const int EC = E / p.nch;
  const int c0 = chunk * EC;
  const int ncol4 = EC >> 2;
  if (ncol4 > 256) {
    // a chunk wider than the block (attn_pick_nch finds no narrower quad-aligned divisor, e.g.
    // E = 4 * prime): each thread owns whole columns and walks the chunk's quads with a stride
    const float* fb = p.feat + (int64_t)b * T * E + c0;
    for (int f4 = tid; f4 < ncol4; f4 += 256) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int t = 0; t < len; ++t) {
        const float w = sE[t];
        const float4 h = *reinterpret_cast<const float4*>(fb + (int64_t)t * E + 4 * f4);
        acc.x = fmaf(w, h.x, acc.x);
        acc.y = fmaf(w, h.y, acc.y);
        acc.z = fmaf(w, h.z, acc.z);
        acc.w = fmaf(w, h.w, acc.w);
      }
      float* cx = p.ctx + (int64_t)b * p.ctx_ld + c0 + 4 * f4;
      cx[0] = acc.x; cx[1] = acc.y; cx[2] = acc.z; cx[3] = acc.w;
    }
    return;
  }
  const int tgc = 256 / ncol4;
  const int f4 = tid % ncol4, tg = tid / ncol4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (tg < tgc) {
    const float* fb = p.feat + (int64_t)b * T * E + c0 + 4 * f4;
    for (int t = tg; t < len; t += tgc) {
      const float w = sE[t];
      const float4 h = *reinterpret_cast<const float4*>(fb + (int64_t)t * E);
      acc.x = fmaf(w, h.x, acc.x);
      acc.y = fmaf(w, h.y, acc.y);
      acc.z = fmaf(w, h.z, acc.z);
      acc.w = fmaf(w, h.w, acc.w);
    }
    *reinterpret_cast<float4*>(sR + tg * EC + 4 * f4) = acc;
  }
  __syncthreads();
  for (int e = tid; e < EC; e += 256) {
    float v = 0.f;
    for (int g = 0; g < tgc; ++g) v += sR[g * EC + e];
    p.ctx[(int64_t)b * p.ctx_ld + c0 + e] = v;
  }
}

// Backward of one step w.r.t. the energies and the query:
//   dalpha[t] = h[b,t,:] . dctx[b,:]
//   de[t]     = alpha[t] * (dalpha[t] - sum_t' alpha[t'] dalpha[t'])
//   dq[a]     = sum_t de[t] comp[b,t,a];   dqpre = dq * (1 - q^2)
// The products that need all steps at once (d comp, d h, d W_phi) are batched
// GEMMs in the caller; ds = dqpre . W_phi rides along the next cell kernel.
struct AttnBwd {
  const float* dctx;     // [B][dctx_ld]
  int64_t dctx_ld;
  const float* datt;     // optional direct derivative of alpha: datt[b * datt_sb + t]
  int64_t datt_sb;
  const float* att;      // att[b * att_sb + t]
  int64_t att_sb;
  const float* q;        // [B][A]
  const float* comp;     // [B][T][A]
  const float* feat;     // [B][T][E]
  const int32_t* lens;
  float* de;             // de[b * de_sb + t]
  int64_t de_sb;
  float* dqpre;          // [B][A]
  int B, T, A, E;
};

// grid (B), 512 threads, dynamic LDS: E + T + 2048 + 16 floats
__global__ __launch_bounds__(512) void attn_step_bwd_kernel(AttnBwd p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int T = p.T, A = p.A, E = p.E;
  float* sD = smem;                         // [E] dctx
  float* sE = sD + E;                       // [T] dalpha -> de
  float* sR = sE + ((T + 3) & ~3);          // [2048]
  float* sW = sR + 2048;                    // [16]
  const int b = blockIdx.x, tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  int len = p.lens ? p.lens[b] : T;
  len = len < T ? len : T;

  for (int e = tid; e < E; e += 512) sD[e] = p.dctx[(int64_t)b * p.dctx_ld + e];
  __syncthreads();
  const float* fb = p.feat + (int64_t)b * T * E;
  for (int t = wave; t < len; t += 8) {
    const float4* row = reinterpret_cast<const float4*>(fb + (int64_t)t * E);
    float acc = 0.f;
    for (int e4 = lane; e4 < (E >> 2); e4 += 64) {
      const float4 h = row[e4];
      const float4 d = *reinterpret_cast<const float4*>(sD + 4 * e4);
      acc = fmaf(h.x, d.x, acc);
      acc = fmaf(h.y, d.y, acc);
      acc = fmaf(h.z, d.z, acc);
      acc = fmaf(h.w, d.w, acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) sE[t] = acc + (p.datt ? p.datt[(int64_t)b * p.datt_sb + t] : 0.f);
  }
  __syncthreads();
  const float* ab = p.att + (int64_t)b * p.att_sb;
  float dot = 0.f;
  for (int t = tid; t < len; t += 512) dot += ab[t] * sE[t];
  dot = block_reduce_sum(dot, sW, 8);
  for (int t = tid; t < T; t += 512) {
    const float v = t < len ? ab[t] * (sE[t] - dot) : 0.f;
    if (t < len) sE[t] = v;
    p.de[(int64_t)b * p.de_sb + t] = v;
  }
  __syncthreads();

  const int ncol4 = A >> 2;
  const int tgc = 512 / ncol4 > 0 ? (512 / ncol4 < 2048 / A ? 512 / ncol4 : 2048 / A) : 1;
  const int a4 = tid % ncol4, tg = tid / ncol4;
  if (tg < tgc) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* cb = p.comp + (int64_t)b * T * A + 4 * a4;
    for (int t = tg; t < len; t += tgc) {
      const float w = sE[t];
      const float4 c = *reinterpret_cast<const float4*>(cb + (int64_t)t * A);
      acc.x = fmaf(w, c.x, acc.x);
      acc.y = fmaf(w, c.y, acc.y);
      acc.z = fmaf(w, c.z, acc.z);
      acc.w = fmaf(w, c.w, acc.w);
    }
    *reinterpret_cast<float4*>(sR + tg * A + 4 * a4) = acc;
  }
  __syncthreads();
  for (int a = tid; a < A; a += 512) {
    float v = 0.f;
    for (int g = 0; g < tgc; ++g) v += sR[g * A + a];
    const float qq = p.q[(int64_t)b * A + a];
    p.dqpre[(int64_t)b * A + a] = v * (1.f - qq * qq);
  }
}

// Next-character choice of the decode loop (src/asr.py:89-100) for the steps
// that are not teacher forced: logits = char_trans(h2), then argmax (mode 2)
// or an inverse-CDF draw from softmax(logits) with a pre-drawn uniform
// (mode 1; Categorical(...).sample() in the reference), then the embedding
// row of the chosen character is copied out as the next step's input.
struct CharSelect {
  const float* h2;       // [B][D]
  const float* wct;      // [V][D]
  const float* bct;      // [V]
  const float* embed;    // [V][D]
  const float* uni;      // [B] uniforms in [0,1) (mode 1)
  int32_t* chars_next;   // [B]
  float* emb_next;       // [B][D]
  int B, D, V, mode;
};

// grid (B), 256 threads, dynamic LDS: V + 16 floats
__global__ __launch_bounds__(256) void char_select_kernel(CharSelect p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sL = smem;
  __shared__ int pick;
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* h = p.h2 + (int64_t)b * p.D;
  for (int v = wave; v < p.V; v += 4) {
    const float* w = p.wct + (int64_t)v * p.D;
    float acc = 0.f;
    for (int k = lane; k < p.D; k += 64) acc = fmaf(w[k], h[k], acc);
    acc = wave_sum(acc);
    if (lane == 0) sL[v] = acc + p.bct[v];
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    float m = sL[0];
    for (int v = 1; v < p.V; ++v)
      if (sL[v] > m) { m = sL[v]; best = v; }
    if (p.mode == 1) {
      float tot = 0.f;
      for (int v = 0; v < p.V; ++v) tot += expf(sL[v] - m);
      const float target = p.uni[b] * tot;
      float run = 0.f;
      best = p.V - 1;
      for (int v = 0; v < p.V; ++v) {
        run += expf(sL[v] - m);
        if (run > target) { best = v; break; }
      }
    }
    pick = best;
    p.chars_next[b] = best;
  }
  __syncthreads();
  const float* er = p.embed + (int64_t)pick * p.D;
  for (int k = tid; k < p.D; k += 256) p.emb_next[(int64_t)b * p.D + k] = er[k];
}

// The characters fed to the decode steps and their embeddings in one pass, rows = (U + 1) * B in
// step-major order: chars[t][b] = t ? teacher[b][t] : 0 (<sos>; teacher may be null) and
// out[row][:] = table[chars[row]][:].  With `modes` (device int32[U]): the rows of step t + 1
// after a step t that is not teacher forced (modes[t] != 0) are produced later, by the
// persistent decode loop, and start as its fill pattern instead.
__global__ void embed_chars_kernel(const float* table, const int32_t* teacher, int64_t ld, int32_t* chars,
                                   float* out, int64_t rows, int D, const int32_t* modes, int B, int U) {
  const int64_t row = blockIdx.x;
  if (row >= rows) return;
  const int64_t t = row / B;
  const int b = (int)(row - t * B);
  const int ch = (t && teacher) ? teacher[(int64_t)b * ld + t] : 0;
  if (threadIdx.x == 0) chars[row] = ch;
  if (modes && t >= 1 && t < U && modes[t - 1] != 0) {
    const float fill = __builtin_bit_cast(float, 0x7FC0DEADu);      // PERSIST_SENTINEL (rnn_kernels.h)
    for (int k = threadIdx.x; k < D; k += blockDim.x) out[row * D + k] = fill;
    return;
  }
  const float* src = table + (int64_t)ch * D;
  for (int k = threadIdx.x; k < D; k += blockDim.x) out[row * D + k] = src[k];
}

// dtable[idx[row]][:] += g[row][:]
__global__ void embed_scatter_add_kernel(const float* g, const int32_t* idx, float* dtable, int64_t rows, int D) {
  const int64_t row = blockIdx.x;
  if (row >= rows) return;
  float* dst = dtable + (int64_t)idx[row] * D;
  for (int k = threadIdx.x; k < D; k += blockDim.x) atomicAdd(dst + k, g[row * D + k]);
}

// dpre = dcomp * (1 - comp^2), in place on dcomp
__global__ void tanh_bwd_kernel(float* dcomp, const float* comp, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float c = comp[i];
    dcomp[i] *= (1.f - c * c);
  }
}

inline size_t attn_fwd_long_lds(int T) { return sizeof(float) * (size_t)(((T + 3) & ~3) + 1024 + 16); }
inline size_t attn_fwd_lds(int A, int T) { return sizeof(float) * (size_t)(A + ((T + 3) & ~3) + 1024 + 16); }
inline size_t attn_bwd_lds(int E, int T) { return sizeof(float) * (size_t)(E + ((T + 3) & ~3) + 2048 + 16); }

inline int attn_pick_nch(int E) {
  int nch = E / 128;
  if (nch < 1) nch = 1;
  while (nch > 1 && (E % nch != 0 || (E / nch) % 4 != 0)) --nch;
  return nch;
}

}  // namespace
