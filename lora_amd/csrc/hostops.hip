// Pointwise / normalisation fusions of the FROZEN host model that the training step
// (training_scripts/train_lora_dreambooth.py:838-892 -> unet(...)) spends its launches on
// between the adapted Linear / Conv2d sites:
//
//   GroupNorm (+ SiLU)   ResnetBlock2D.norm1/norm2 + nonlinearity, Transformer2DModel.norm, conv_norm_out
//                        ATen: 4 launches forward (moments, fused params, normalise, silu), 5 backward, and it
//                        keeps the normalised tensor AND the SiLU input alive for backward.
//                        Here: NCHW 2 launches each way (slice statistics, apply), only x and [B,G] (mean, rstd) kept;
//                        channels_last 3 each way (statistics, finalize, apply), or ONE where a bundle of groups fits in
//                        a workgroup's registers (maps up to 32x32); only x and the per-channel aff [B,4,C] kept.
//                        The channels_last backward takes a second gradient of x (gsum: the shortcut of a ResnetBlock2D, the
//                        closing residual of a Transformer2DModel) and adds it in the launch that writes dx.
//   ResnetBlock2D tail   conv2 bias, conv_shortcut bias and shortcut + h: three ATen adds -> one launch with their roundings.
//   GEGLU gate           GEGLU.forward right behind the adapted `proj` (lora_diffusion/lora.py:14 targets GEGLU):
//                        h * gelu(gate): ATen = chunk, gelu, mul (5 tensor passes) forward and
//                        gelu_backward, 2 mul, cat (13 passes) backward.  Here: one launch each way (3 / 5 passes);
//                        the backward writes the [M, 2*inner] gradient in place of the cat, which is exactly the G
//                        operand the adapter backward kernels stream next.
//
// All of it is HBM-bound streaming with 16-byte lanes; reductions are per (sample, group) and split into slices so
// that ~1000 workgroups are in flight even when B*G = 128.  Affine parameters are frozen (the reference trains only
// the LoRA factors), so no dgamma / dbeta is produced; callers that train them must use the library path.
#include <algorithm>
#include <atomic>

#include "common.hpp"

namespace lora_amd {

constexpr int kHT = 256;       // threads per workgroup
constexpr int kHU = 4;         // 16-byte chunks per thread held in registers
constexpr int kHMaxSlices = 256;

__device__ inline float fast_rcp(float v) { return __builtin_amdgcn_rcpf(v); }
__device__ inline float sigmoidf(float z) { return fast_rcp(1.f + __expf(-z)); }
// d/dz [z * sigmoid(z)]
__device__ inline float silu_grad(float z) {
  const float s = sigmoidf(z);
  return s * (1.f + z * (1.f - s));
}
// erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7, below f32 round-off of the products it feeds)
__device__ inline float erf_as(float x) {
  const float ax = fabsf(x);
  const float t = fast_rcp(1.f + 0.3275911f * ax);
  float p = 1.061405429f;
  p = fmaf(p, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  const float e = 1.f - p * t * __expf(-ax * ax);
  return copysignf(e, x);
}
__device__ inline float gelu_cdf(float g) { return 0.5f * (1.f + erf_as(g * 0.70710678118654752f)); }
__device__ inline float gelu_pdf(float g) { return 0.39894228040143268f * __expf(-0.5f * g * g); }

// Sum of two per-thread values over the workgroup; every thread receives both totals.
__device__ inline void block_sum2(float &a, float &b, float (*s)[2]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();  // previous use of s is over
  if (lane == 0) { s[wave][0] = a; s[wave][1] = b; }
  __syncthreads();
  a = (s[0][0] + s[1][0]) + (s[2][0] + s[3][0]);
  b = (s[0][1] + s[1][1]) + (s[2][1] + s[3][1]);
}

// One (sample, group) = `chunks` consecutive 16-byte chunks of an NCHW tensor, cut into S slices of `per_block`.
struct GnGeo {
  int cpg, chunks, per_block, S;
  int64_t span;
  bool ok;
};
static GnGeo gn_geo(int B, int C, int HW, int G) {
  GnGeo q{};
  q.ok = B > 0 && C > 0 && HW > 0 && G > 0 && C % G == 0 && HW % 8 == 0;
  if (!q.ok) return q;
  q.cpg = C / G;
  q.span = (int64_t)q.cpg * HW;
  q.ok = q.span / 8 <= (int64_t)kHMaxSlices * kHT * kHU;
  if (!q.ok) return q;
  q.chunks = (int)(q.span / 8);
  int64_t pb = (int64_t)B * G * q.chunks / 1024;  // aim at ~1000 workgroups
  pb = std::max<int64_t>(64, std::min<int64_t>(pb, kHT * kHU));
  pb = std::min<int64_t>(pb, q.chunks);
  q.per_block = (int)pb;
  q.S = (q.chunks + q.per_block - 1) / q.per_block;
  return q;
}

struct GnBlock {
  int64_t bg;       // sample * G + group
  int slice, nloc;  // slice index, chunks in this slice
  int64_t base;     // first element of the slice in the tensor
  int c0;           // first channel of the group
};
__device__ inline GnBlock gn_block(int G, int cpg, int HW, int chunks, int per_block, int S) {
  GnBlock b;
  b.bg = blockIdx.x / S;
  b.slice = (int)(blockIdx.x - b.bg * S);
  b.nloc = min(per_block, chunks - b.slice * per_block);
  b.base = b.bg * (int64_t)cpg * HW + (int64_t)b.slice * per_block * 8;
  b.c0 = (int)(b.bg % G) * cpg;
  return b;
}

// gamma / beta of the channel each of the thread's chunks lies in (HW % 8 == 0: a chunk never straddles channels).
// Loaded up front, next to the activation loads, so that nothing later waits on a dependent scalar fetch.
template <class E>
__device__ inline void gn_load_affine(const typename E::storage *__restrict__ gamma,
                                      const typename E::storage *__restrict__ beta, const GnBlock &b, int per_block,
                                      int HW, float (&ga)[kHU], float (&be)[kHU]) {
#pragma unroll
  for (int u = 0; u < kHU; ++u) {
    const int i = threadIdx.x + u * kHT;
    const int c = b.c0 + ((b.slice * per_block + (i < b.nloc ? i : 0)) * 8) / HW;
    ga[u] = E::to_f(gamma[c]);
    be[u] = E::to_f(beta[c]);
  }
}
// Keep the compiler from sinking loads below (or hoisting their consumers above) this point: without it hipcc
// consumes the first chunk before issuing the second load, i.e. one HBM round trip per chunk.
#define LORA_AMD_LOADS_ISSUED() __builtin_amdgcn_sched_barrier(0)

// ---- GroupNorm forward ---------------------------------------------------------------------------------------------
// Stage 1: slice mean and M2 = sum (x - slice mean)^2 with the slice held in registers (no E[x^2] - mean^2
// cancellation).  part[bg][slice] = (mean, M2); the slice's element count follows from the geometry.
template <class E>
__global__ __launch_bounds__(kHT) void gn_stats_kernel(const typename E::storage *__restrict__ x,
                                                       float *__restrict__ part, int G, int cpg, int HW, int chunks,
                                                       int per_block, int S) {
  __shared__ float s_red[4][2];
  const GnBlock b = gn_block(G, cpg, HW, chunks, per_block, S);
  const int tid = threadIdx.x;
  float v[kHU][8];
  float sum = 0.f, zero = 0.f;
  Raw8<E> raw[kHU];
#pragma unroll
  for (int u = 0; u < kHU; ++u) {
    const int i = tid + u * kHT;
    raw[u] = load8_raw<E>(x + b.base + (int64_t)(i < b.nloc ? i : 0) * 8);
  }
  LORA_AMD_LOADS_ISSUED();
#pragma unroll
  for (int u = 0; u < kHU; ++u) {
    unpack8_sel<E>(raw[u], tid + u * kHT < b.nloc, v[u]);
#pragma unroll
    for (int e = 0; e < 8; ++e) sum += v[u][e];
  }
  block_sum2(sum, zero, s_red);
  const float mean = sum / (float)(b.nloc * 8);
  float m2 = 0.f;
  zero = 0.f;
#pragma unroll
  for (int u = 0; u < kHU; ++u) {
    if (tid + u * kHT < b.nloc) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = v[u][e] - mean;
        m2 = fmaf(d, d, m2);
      }
    }
  }
  block_sum2(m2, zero, s_red);
  if (tid == 0) {
    part[(b.bg * S + b.slice) * 2 + 0] = mean;
    part[(b.bg * S + b.slice) * 2 + 1] = m2;
  }
}

// Stage 2: merge the S slice statistics (Chan et al.), normalise, affine, optional SiLU.
template <class E, bool ACT>
__global__ __launch_bounds__(kHT) void gn_apply_kernel(const typename E::storage *__restrict__ x,
                                                       const typename E::storage *__restrict__ gamma,
                                                       const typename E::storage *__restrict__ beta,
                                                       typename E::storage *__restrict__ y,
                                                       const float *__restrict__ part, float *__restrict__ stats,
                                                       int G, int cpg, int HW, int chunks, int per_block, int S,
                                                       float eps) {
  __shared__ float s_red[4][2];
  const GnBlock b = gn_block(G, cpg, HW, chunks, per_block, S);
  const int tid = threadIdx.x;
  // issue the slice's loads first; the statistics merge below overlaps their latency
  Raw8<E> raw[kHU];
#pragma unroll
  for (int u = 0; u < kHU; ++u) {
    const int i = tid + u * kHT;
    raw[u] = load8_raw<E>(x + b.base + (int64_t)(i < b.nloc ? i : 0) * 8);
  }
  float gam[kHU], bet[kHU];
  gn_load_affine<E>(gamma, beta, b, per_block, HW, gam, bet);
  const float n_all = (float)chunks * 8.f;
  const int ts = tid < S ? tid : 0;
  const float n_t = tid < S ? 8.f * (float)min(per_block, chunks - ts * per_block) : 0.f;
  const float mean_t = part[(b.bg * S + ts) * 2 + 0];
  const float m2_t = tid < S ? part[(b.bg * S + ts) * 2 + 1] : 0.f;
  LORA_AMD_LOADS_ISSUED();
  float a = n_t * mean_t, zero = 0.f;
  block_sum2(a, zero, s_red);
  const float mean = a / n_all;
  const float dm = mean_t - mean;
  float m2 = fmaf(n_t * dm, dm, m2_t);
  zero = 0.f;
  block_sum2(m2, zero, s_red);
  const float rstd = rsqrtf(m2 / n_all + eps);
  if (b.slice == 0 && tid == 0) {
    stats[b.bg * 2 + 0] = mean;
    stats[b.bg * 2 + 1] = rstd;
  }
#pragma unroll
  for (int u = 0; u < kHU; ++u) {
    const int i = tid + u * kHT;
    if (i < b.nloc) {
      const float ga = gam[u] * rstd;
      const float be = fmaf(-mean, ga, bet[u]);
      float o[8], v[8];
      unpack8_sel<E>(raw[u], true, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float z = fmaf(v[e], ga, be);
        o[e] = ACT ? z * sigmoidf(z) : z;
      }
      store8<E>(y + b.base + (int64_t)i * 8, o);
    }
  }
}

// ---- GroupNorm backward (input gradient only: gamma / beta are frozen) --------------------------------------------
// t = gamma * dL/dz,  xh = (x - mean) * rstd;  dx = rstd * (t - mean_g(t) - xh * mean_g(t * xh)).
template <class E, bool ACT>
__device__ inline void gn_bwd_terms(const float (&xv)[8], const float (&gv)[8], float ga_r, float be, float gam,
                                    float mean, float rstd, float (&t)[8], float (&xh)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    xh[e] = (xv[e] - mean) * rstd;
    float dz = gv[e];
    if (ACT) dz *= silu_grad(fmaf(xv[e], ga_r, be));
    t[e] = gam * dz;
  }
}

template <class E, bool ACT>
__global__ __launch_bounds__(kHT) void gn_bwd_stats_kernel(const typename E::storage *__restrict__ x,
                                                           const typename E::storage *__restrict__ gout,
                                                           const typename E::storage *__restrict__ gamma,
                                                           const typename E::storage *__restrict__ beta,
                                                           const float *__restrict__ stats, float *__restrict__ part,
                                                           int G, int cpg, int HW, int chunks, int per_block, int S) {
  __shared__ float s_red[4][2];
  const GnBlock b = gn_block(G, cpg, HW, chunks, per_block, S);
  const int tid = threadIdx.x;
  Raw8<E> xr[kHU], gr[kHU];
#pragma unroll
  for (int u = 0; u < kHU; ++u) {
    const int i = tid + u * kHT;
    const int64_t off = b.base + (int64_t)(i < b.nloc ? i : 0) * 8;
    xr[u] = load8_raw<E>(x + off);
    gr[u] = load8_raw<E>(gout + off);
  }
  float gam[kHU], bet[kHU];
  gn_load_affine<E>(gamma, beta, b, per_block, HW, gam, bet);
  const float mean = stats[b.bg * 2 + 0], rstd = stats[b.bg * 2 + 1];
  LORA_AMD_LOADS_ISSUED();
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int u = 0; u < kHU; ++u) {
    const int i = tid + u * kHT;
    if (i < b.nloc) {
      const float ga_r = gam[u] * rstd, be = fmaf(-mean, ga_r, bet[u]);
      float t[8], xh[8], xv[8], gv[8];
      unpack8_sel<E>(xr[u], true, xv);
      unpack8_sel<E>(gr[u], true, gv);
      gn_bwd_terms<E, ACT>(xv, gv, ga_r, be, gam[u], mean, rstd, t, xh);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        s1 += t[e];
        s2 = fmaf(t[e], xh[e], s2);
      }
    }
  }
  block_sum2(s1, s2, s_red);
  if (tid == 0) {
    part[(b.bg * S + b.slice) * 2 + 0] = s1;
    part[(b.bg * S + b.slice) * 2 + 1] = s2;
  }
}

template <class E, bool ACT>
__global__ __launch_bounds__(kHT) void gn_bwd_apply_kernel(const typename E::storage *__restrict__ x,
                                                           const typename E::storage *__restrict__ gout,
                                                           const typename E::storage *__restrict__ gamma,
                                                           const typename E::storage *__restrict__ beta,
                                                           const float *__restrict__ stats,
                                                           const float *__restrict__ part,
                                                           typename E::storage *__restrict__ dx, int G, int cpg,
                                                           int HW, int chunks, int per_block, int S) {
  __shared__ float s_red[4][2];
  const GnBlock b = gn_block(G, cpg, HW, chunks, per_block, S);
  const int tid = threadIdx.x;
  Raw8<E> xr[kHU], gr[kHU];
#pragma unroll
  for (int u = 0; u < kHU; ++u) {
    const int i = tid + u * kHT;
    const int64_t off = b.base + (int64_t)(i < b.nloc ? i : 0) * 8;
    xr[u] = load8_raw<E>(x + off);
    gr[u] = load8_raw<E>(gout + off);
  }
  float gam[kHU], bet[kHU];
  gn_load_affine<E>(gamma, beta, b, per_block, HW, gam, bet);
  const int ts = tid < S ? tid : 0;
  float s1 = part[(b.bg * S + ts) * 2 + 0], s2 = part[(b.bg * S + ts) * 2 + 1];
  const float mean = stats[b.bg * 2 + 0], rstd = stats[b.bg * 2 + 1];
  LORA_AMD_LOADS_ISSUED();
  if (tid >= S) s1 = s2 = 0.f;
  block_sum2(s1, s2, s_red);
  const float inv_n = 1.f / ((float)chunks * 8.f);
  const float c1 = s1 * inv_n, c2 = s2 * inv_n;
#pragma unroll
  for (int u = 0; u < kHU; ++u) {
    const int i = tid + u * kHT;
    if (i < b.nloc) {
      const float ga_r = gam[u] * rstd, be = fmaf(-mean, ga_r, bet[u]);
      float t[8], xh[8], o[8], xv[8], gv[8];
      unpack8_sel<E>(xr[u], true, xv);
      unpack8_sel<E>(gr[u], true, gv);
      gn_bwd_terms<E, ACT>(xv, gv, ga_r, be, gam[u], mean, rstd, t, xh);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = rstd * (t[e] - c1 - xh[e] * c2);
      store8<E>(dx + b.base + (int64_t)i * 8, o);
    }
  }
}

// ---- GEGLU gate ----------------------------------------------------------------------------------------------------
// y = [h | gate] per row (2 * inner columns);  out = h * gelu(gate)   (exact erf form, F.gelu's default).
template <class E>
__global__ __launch_bounds__(kHT) void geglu_fwd_kernel(const typename E::storage *__restrict__ y, int64_t ldy,
                                                        typename E::storage *__restrict__ out, int64_t ldo,
                                                        int64_t M, int c8) {
  const uint32_t total = (uint32_t)(M * c8);  // host checks M * c8 < 2^31
  const uint32_t i0 = blockIdx.x * (uint32_t)(kHT * kHU) + threadIdx.x;
  Raw8<E> hr[kHU], gr[kHU];
  int64_t rows[kHU];
  int cols[kHU];
  const uint32_t dq = (uint32_t)kHT / (uint32_t)c8, dr = (uint32_t)kHT % (uint32_t)c8;
  const uint32_t row0 = min(i0, total - 1) / (uint32_t)c8, col0 = min(i0, total - 1) - row0 * (uint32_t)c8;
  uint32_t row = row0, col = col0;
#pragma unroll
  for (int u = 0; u < kHU; ++u) {
    const bool ok = i0 + u * kHT < total;  // chunks past the end re-read the block's first chunk
    rows[u] = ok ? row : row0;
    cols[u] = (int)(ok ? col : col0) * 8;
    row += dq; col += dr;
    if (col >= (uint32_t)c8) { col -= c8; ++row; }
    const typename E::storage *p = y + rows[u] * ldy + cols[u];
    hr[u] = load8_raw<E>(p);
    gr[u] = load8_raw<E>(p + (int64_t)c8 * 8);
  }
  LORA_AMD_LOADS_ISSUED();
#pragma unroll
  for (int u = 0; u < kHU; ++u) {
    if (i0 + u * kHT < total) {
      float o[8], h[8], g[8];
      unpack8_sel<E>(hr[u], true, h);
      unpack8_sel<E>(gr[u], true, g);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = h[e] * (g[e] * gelu_cdf(g[e]));
      store8<E>(out + rows[u] * ldo + cols[u], o);
    }
  }
}

// gy[:, :inner] = gout * gelu(gate);  gy[:, inner:] = gout * h * gelu'(gate)
template <class E>
__global__ __launch_bounds__(kHT) void geglu_bwd_kernel(const typename E::storage *__restrict__ y, int64_t ldy,
                                                        const typename E::storage *__restrict__ gout, int64_t ldg,
                                                        typename E::storage *__restrict__ gy, int64_t ldgy,
                                                        int64_t M, int c8) {
  constexpr int U = 2;
  const uint32_t total = (uint32_t)(M * c8);  // host checks M * c8 < 2^31
  const uint32_t i0 = blockIdx.x * (uint32_t)(kHT * U) + threadIdx.x;
  Raw8<E> hr[U], gr[U], gor[U];
  int64_t rows[U];
  int cols[U];
  const uint32_t dq = (uint32_t)kHT / (uint32_t)c8, dr = (uint32_t)kHT % (uint32_t)c8;
  const uint32_t row0 = min(i0, total - 1) / (uint32_t)c8, col0 = min(i0, total - 1) - row0 * (uint32_t)c8;
  uint32_t row = row0, col = col0;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const bool ok = i0 + u * kHT < total;
    rows[u] = ok ? row : row0;
    cols[u] = (int)(ok ? col : col0) * 8;
    row += dq; col += dr;
    if (col >= (uint32_t)c8) { col -= c8; ++row; }
    const typename E::storage *p = y + rows[u] * ldy + cols[u];
    hr[u] = load8_raw<E>(p);
    gr[u] = load8_raw<E>(p + (int64_t)c8 * 8);
    gor[u] = load8_raw<E>(gout + rows[u] * ldg + cols[u]);
  }
  LORA_AMD_LOADS_ISSUED();
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (i0 + u * kHT < total) {
      float dh[8], dg[8], h[8], g[8], go[8];
      unpack8_sel<E>(hr[u], true, h);
      unpack8_sel<E>(gr[u], true, g);
      unpack8_sel<E>(gor[u], true, go);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float cdf = gelu_cdf(g[e]);
        dh[e] = go[e] * (g[e] * cdf);
        dg[e] = go[e] * h[e] * fmaf(g[e], gelu_pdf(g[e]), cdf);
      }
      typename E::storage *q = gy + rows[u] * ldgy + cols[u];
      store8<E>(q, dh);
      store8<E>(q + (int64_t)c8 * 8, dg);
    }
  }
}

// ---- LayerNorm over the last dimension (BasicTransformerBlock.norm1/2/3) -----------------------------------------
// One row = K/8 chunks spread over L = 2^logL consecutive lanes (<= kLU chunks per lane, all in registers); a wave
// holds 64/L rows.  Mean, then M2 around it, by xor-shuffles inside the lane group: one launch forward, one backward
// (ATen: 24 us / 34 us per call at [16384, 320] bf16, i.e. < 1 TB/s).
constexpr int kLU = 5;

__device__ inline float group_allsum(float v, int logL) {
  for (int off = 1; off < (1 << logL); off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ADD: the row is x + res (the residual add in front of norm2 / norm3), rounded to the activation dtype exactly as the
// separate add would, written to sum_out for the residual stream, and normalised in the same pass.
template <class E, bool ADD>
__global__ __launch_bounds__(kHT) void ln_fwd_kernel(const typename E::storage *__restrict__ x,
                                                     const typename E::storage *__restrict__ res,
                                                     const typename E::storage *__restrict__ gamma,
                                                     const typename E::storage *__restrict__ beta,
                                                     typename E::storage *__restrict__ sum_out,
                                                     typename E::storage *__restrict__ y, float *__restrict__ stats,
                                                     int64_t M, int c8, int logL, float eps) {
  const int L = 1 << logL, l = threadIdx.x & (L - 1);
  const int64_t row = (int64_t)blockIdx.x * (kHT >> logL) + (threadIdx.x >> logL);
  const bool live = row < M;
  const int64_t rbase = (live ? row : 0) * (int64_t)c8 * 8;
  const typename E::storage *xr = x + rbase;
  Raw8<E> raw[kLU], rr[ADD ? kLU : 1], gr[kLU], br[kLU];
#pragma unroll
  for (int u = 0; u < kLU; ++u) {
    const int cc = l + u * L, cs = cc < c8 ? cc : l;
    raw[u] = load8_raw<E>(xr + cs * 8);
    if (ADD) rr[u] = load8_raw<E>(res + rbase + cs * 8);
    gr[u] = load8_raw<E>(gamma + cs * 8);
    br[u] = load8_raw<E>(beta + cs * 8);
  }
  LORA_AMD_LOADS_ISSUED();
  float v[kLU][8], sum = 0.f;
#pragma unroll
  for (int u = 0; u < kLU; ++u) {
    const bool ok = l + u * L < c8;
    unpack8_sel<E>(raw[u], ok, v[u]);
    if (ADD) {
      float rv[8];
      unpack8_sel<E>(rr[u], ok, rv);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[u][e] = round_to<E>(v[u][e] + rv[e]);
      if (ok && live) store8<E>(sum_out + row * (int64_t)c8 * 8 + (l + u * L) * 8, v[u]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) sum += v[u][e];
  }
  const float inv_n = 1.f / (float)(c8 * 8);
  const float mean = group_allsum(sum, logL) * inv_n;
  float m2 = 0.f;
#pragma unroll
  for (int u = 0; u < kLU; ++u)
    if (l + u * L < c8) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = v[u][e] - mean;
        m2 = fmaf(d, d, m2);
      }
    }
  const float rstd = rsqrtf(group_allsum(m2, logL) * inv_n + eps);
  if (!live) return;
  if (l == 0) {
    stats[row * 2 + 0] = mean;
    stats[row * 2 + 1] = rstd;
  }
#pragma unroll
  for (int u = 0; u < kLU; ++u) {
    const int cc = l + u * L;
    if (cc < c8) {
      float ga[8], be[8], o[8];
      unpack8_sel<E>(gr[u], true, ga);
      unpack8_sel<E>(br[u], true, be);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = fmaf((v[u][e] - mean) * rstd, ga[e], be[e]);
      store8<E>(y + row * (int64_t)c8 * 8 + cc * 8, o);
    }
  }
}

// dx = rstd * (t - mean(t) - xh * mean(t * xh)),  t = gamma * gout,  xh = (x - mean) * rstd   (gamma / beta frozen)
// ADDG: dx additionally receives gsum, the gradient that reaches the same row through the residual stream.
template <class E, bool ADDG>
__global__ __launch_bounds__(kHT) void ln_bwd_kernel(const typename E::storage *__restrict__ x,
                                                     const typename E::storage *__restrict__ gout,
                                                     const typename E::storage *__restrict__ gsum,
                                                     const typename E::storage *__restrict__ gamma,
                                                     const float *__restrict__ stats,
                                                     typename E::storage *__restrict__ dx, int64_t M, int c8,
                                                     int logL) {
  const int L = 1 << logL, l = threadIdx.x & (L - 1);
  const int64_t row = (int64_t)blockIdx.x * (kHT >> logL) + (threadIdx.x >> logL);
  const bool live = row < M;
  const int64_t rbase = (live ? row : 0) * (int64_t)c8 * 8;
  Raw8<E> xr[kLU], gor[kLU], gsr[ADDG ? kLU : 1], gr[kLU];
#pragma unroll
  for (int u = 0; u < kLU; ++u) {
    const int cc = l + u * L, cs = cc < c8 ? cc : l;
    xr[u] = load8_raw<E>(x + rbase + cs * 8);
    gor[u] = load8_raw<E>(gout + rbase + cs * 8);
    if (ADDG) gsr[u] = load8_raw<E>(gsum + rbase + cs * 8);
    gr[u] = load8_raw<E>(gamma + cs * 8);
  }
  const float mean = stats[(live ? row : 0) * 2 + 0], rstd = stats[(live ? row : 0) * 2 + 1];
  LORA_AMD_LOADS_ISSUED();
  float t[kLU][8], xh[kLU][8], s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int u = 0; u < kLU; ++u) {
    const bool ok = l + u * L < c8;
    float xv[8], gv[8], ga[8];
    unpack8_sel<E>(xr[u], ok, xv);
    unpack8_sel<E>(gor[u], ok, gv);
    unpack8_sel<E>(gr[u], ok, ga);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      xh[u][e] = ok ? (xv[e] - mean) * rstd : 0.f;
      t[u][e] = ga[e] * gv[e];
      s1 += t[u][e];
      s2 = fmaf(t[u][e], xh[u][e], s2);
    }
  }
  const float inv_n = 1.f / (float)(c8 * 8);
  const float c1 = group_allsum(s1, logL) * inv_n, c2 = group_allsum(s2, logL) * inv_n;
  if (!live) return;
#pragma unroll
  for (int u = 0; u < kLU; ++u) {
    const int cc = l + u * L;
    if (cc < c8) {
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = rstd * (t[u][e] - c1 - xh[u][e] * c2);
      if (ADDG) {
        float gs[8];
        unpack8_sel<E>(gsr[u], true, gs);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += gs[e];
      }
      store8<E>(dx + row * (int64_t)c8 * 8 + cc * 8, o);
    }
  }
}

// lanes per row: the smallest power of two that leaves <= kLU chunks per lane (-1: row too long)
static inline int ln_logL(int c8) {
  for (int lg = 0; lg <= 6; ++lg)
    if (((c8 + (1 << lg) - 1) >> lg) <= kLU) return lg;
  return -1;
}

// ---- GroupNorm on channels_last (NHWC) activations -------------------------------------------------------------------
// Memory is [B][HW][C]: a group is C/G adjacent channels of every pixel, so the reduction runs over pixels.  Every
// streaming kernel uses a column-owner mapping: thread = (pixel slot, 16-byte channel chunk), the chunk is fixed for
// the thread's lifetime (its per-channel vectors are loaded once), consecutive lanes read consecutive chunks of one
// pixel (contiguous runs of cw * 16 bytes).  Statistics are per channel and per pixel slice (shifted sums -> mean, M2),
// a tiny finalize kernel folds slices and the group's channels together (Chan) and expands the result per channel:
//   aff[b][0][c] = gamma*rstd, aff[b][1][c] = beta - mean*gamma*rstd, aff[b][2][c] = mean, aff[b][3][c] = rstd
// so that the apply kernels are pure per-channel affine maps.  3 + 3 launches (1 + 1 on the maps the resident form further
// down holds); MIOpen's NHWC kernels then need no
// NCHW<->NHWC transposes around them and the transformer blocks read the activations as tokens without a copy.
constexpr int kNU = 4;  // pixels in flight per thread

struct GnNhwcGeo {
  int c8, cw, tiles, nslots, px, S;
  bool ok;
};
static GnNhwcGeo gn_nhwc_geo(int B, int C, int HW, int G) {
  GnNhwcGeo q{};
  q.ok = B > 0 && C > 0 && HW > 0 && G > 0 && C % G == 0 && C % 8 == 0;
  if (!q.ok) return q;
  q.c8 = C / 8;
  int best = 1, best_act = 0;
  for (int d = 1; d <= std::min(q.c8, 128); ++d) {
    if (q.c8 % d) continue;
    const int act = (kHT / d) * d;
    if (act >= best_act) { best_act = act; best = d; }
  }
  q.cw = best;
  q.tiles = q.c8 / q.cw;
  q.nslots = kHT / q.cw;
  // pixels per workgroup: ~768 workgroups on the large maps, at least two pixels per slot on the small ones (the
  // per-channel partials are 8 bytes per channel and slice: keep them a small fraction of the stream)
  int64_t px = std::max<int64_t>(2 * q.nslots, (int64_t)HW * B * q.tiles / 768);
  px = std::min<int64_t>(px, HW);
  q.px = (int)px;
  q.S = (HW + q.px - 1) / q.px;
  return q;
}

struct NhwcBlock {
  int b, s, col, slot, np;
  bool active;
  int64_t base;  // element offset of (b, first pixel of the slice, this thread's chunk)
};
__device__ inline NhwcBlock nhwc_block(int C, int HW, int cw, int tiles, int nslots, int px, int S) {
  NhwcBlock k;
  const int bs = blockIdx.x / tiles, tile = blockIdx.x - bs * tiles;
  k.b = bs / S;
  k.s = bs - k.b * S;
  k.slot = threadIdx.x / cw;
  const int cl = threadIdx.x - k.slot * cw;
  k.active = k.slot < nslots;
  k.col = tile * cw + cl;
  const int p0 = k.s * px;
  k.np = min(px, HW - p0);
  k.base = ((int64_t)k.b * HW + p0) * C + (int64_t)k.col * 8;
  return k;
}

__device__ inline void ld8f(const float *p, float (&v)[8]) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  const f4 a = *reinterpret_cast<const f4 *>(p), b = *reinterpret_cast<const f4 *>(p + 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) { v[i] = a[i]; v[i + 4] = b[i]; }
}
__device__ inline void st8f(float *p, const float (&v)[8]) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  f4 a, b;
#pragma unroll
  for (int i = 0; i < 4; ++i) { a[i] = v[i]; b[i] = v[i + 4]; }
  *reinterpret_cast<f4 *>(p) = a;
  *reinterpret_cast<f4 *>(p + 4) = b;
}

// Sum acc0 / acc1 (8 channels each) over the pixel slots of the block; slot 0 receives the totals.
__device__ inline void nhwc_slot_reduce(float (&a0)[8], float (&a1)[8], const NhwcBlock &k, int cw, int nslots,
                                        float *s_red /* [2][kHT][8] */) {
  if (k.active) {
    st8f(s_red + (size_t)threadIdx.x * 8, a0);
    st8f(s_red + (size_t)(kHT + threadIdx.x) * 8, a1);
  }
  __syncthreads();
  if (k.active && k.slot == 0) {
    for (int sl = 1; sl < nslots; ++sl) {
      float t0[8], t1[8];
      ld8f(s_red + (size_t)(sl * cw + threadIdx.x) * 8, t0);
      ld8f(s_red + (size_t)(kHT + sl * cw + threadIdx.x) * 8, t1);
#pragma unroll
      for (int e = 0; e < 8; ++e) { a0[e] += t0[e]; a1[e] += t1[e]; }
    }
  }
}

// part[((b*S + s)*2 + 0)*C + c] = slice mean of channel c, [.. + 1] = slice M2
template <class E>
__global__ __launch_bounds__(kHT) void gn_nhwc_stats_kernel(const typename E::storage *__restrict__ x,
                                                            float *__restrict__ part, int C, int HW, int cw, int tiles,
                                                            int nslots, int px, int S) {
  __shared__ __attribute__((aligned(16))) float s_red[2 * kHT * 8];
  const NhwcBlock k = nhwc_block(C, HW, cw, tiles, nslots, px, S);
  float sh[8], s1[8], s2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s1[e] = s2[e] = 0.f;
  if (k.active) {
    unpack8_sel<E>(load8_raw<E>(x + k.base), true, sh);  // shift = the slice's first pixel (same for every slot)
    for (int p = k.slot; p < k.np; p += nslots * kNU) {
      Raw8<E> raw[kNU];
#pragma unroll
      for (int u = 0; u < kNU; ++u) {
        const int pp = p + u * nslots;
        raw[u] = load8_raw<E>(x + k.base + (int64_t)(pp < k.np ? pp : p) * C);
      }
      LORA_AMD_LOADS_ISSUED();
#pragma unroll
      for (int u = 0; u < kNU; ++u) {
        float v[8];
        unpack8_sel<E>(raw[u], true, v);
        if (p + u * nslots < k.np) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float d = v[e] - sh[e];
            s1[e] += d;
            s2[e] = fmaf(d, d, s2[e]);
          }
        }
      }
    }
  }
  nhwc_slot_reduce(s1, s2, k, cw, nslots, s_red);
  if (k.active && k.slot == 0) {
    const float inv_n = 1.f / (float)k.np;
    float mean[8], m2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      mean[e] = sh[e] + s1[e] * inv_n;
      m2[e] = fmaxf(s2[e] - s1[e] * s1[e] * inv_n, 0.f);
    }
    float *o = part + ((int64_t)(k.b * S + k.s) * 2) * C + (int64_t)k.col * 8;
    st8f(o, mean);
    st8f(o + C, m2);
  }
}

// One workgroup per (sample, group): fold slices x channels, expand per channel.  `addend` [B][C] (f32, may be null)
// is a per-(sample, channel) term added to x BEFORE the normalisation (ResnetBlock2D: the time-embedding projection and
// the bias of the convolution that produced x).  A per-channel shift moves only the channel means, so it costs nothing
// in the streaming kernels: slice means are shifted here, and the expanded affine absorbs it,
//   z = ((x + add) - mean) * rstd * gamma + beta = x * a + (beta + (add - mean) * a),   xh = (x - (mean - add)) * rstd.
template <class E>
__global__ __launch_bounds__(kHT) void gn_nhwc_finalize_kernel(const float *__restrict__ part,
                                                               const typename E::storage *__restrict__ gamma,
                                                               const typename E::storage *__restrict__ beta,
                                                               const float *__restrict__ addend,
                                                               float *__restrict__ aff, int C, int HW, int G, int px,
                                                               int S, float eps) {
  __shared__ float s_red[4][2];
  const int b = blockIdx.x / G, g = blockIdx.x - b * G, cpg = C / G;
  const int items = S * cpg;
  float a = 0.f, zero = 0.f;
  for (int i = threadIdx.x; i < items; i += kHT) {
    const int s = i / cpg, c = g * cpg + (i - s * cpg);
    const float add = addend != nullptr ? addend[(int64_t)b * C + c] : 0.f;
    a += (float)min(px, HW - s * px) * (part[((int64_t)(b * S + s) * 2) * C + c] + add);
  }
  block_sum2(a, zero, s_red);
  const float n_all = (float)HW * (float)cpg;
  const float mean = a / n_all;
  float m2 = 0.f;
  zero = 0.f;
  for (int i = threadIdx.x; i < items; i += kHT) {
    const int s = i / cpg, c = g * cpg + (i - s * cpg);
    const float *pp = part + ((int64_t)(b * S + s) * 2) * C + c;
    const float add = addend != nullptr ? addend[(int64_t)b * C + c] : 0.f;
    const float dm = pp[0] + add - mean;
    m2 += pp[C] + (float)min(px, HW - s * px) * dm * dm;
  }
  block_sum2(m2, zero, s_red);
  const float rstd = rsqrtf(m2 / n_all + eps);
  for (int cc = threadIdx.x; cc < cpg; cc += kHT) {
    const int c = g * cpg + cc;
    const float add = addend != nullptr ? addend[(int64_t)b * C + c] : 0.f;
    const float ga = E::to_f(gamma[c]) * rstd;
    float *o = aff + (int64_t)b * 4 * C + c;
    o[0] = ga;
    o[C] = fmaf(add - mean, ga, E::to_f(beta[c]));
    o[2 * C] = mean - add;
    o[3 * C] = rstd;
  }
}

template <class E, bool ACT>
__global__ __launch_bounds__(kHT) void gn_nhwc_apply_kernel(const typename E::storage *__restrict__ x,
                                                            const float *__restrict__ aff,
                                                            typename E::storage *__restrict__ y, int C, int HW, int cw,
                                                            int tiles, int nslots, int px, int S) {
  const NhwcBlock k = nhwc_block(C, HW, cw, tiles, nslots, px, S);
  if (!k.active) return;
  float ga[8], be[8];
  ld8f(aff + (int64_t)k.b * 4 * C + (int64_t)k.col * 8, ga);
  ld8f(aff + (int64_t)k.b * 4 * C + C + (int64_t)k.col * 8, be);
  for (int p = k.slot; p < k.np; p += nslots * kNU) {
    Raw8<E> raw[kNU];
#pragma unroll
    for (int u = 0; u < kNU; ++u) {
      const int pp = p + u * nslots;
      raw[u] = load8_raw<E>(x + k.base + (int64_t)(pp < k.np ? pp : p) * C);
    }
    LORA_AMD_LOADS_ISSUED();
#pragma unroll
    for (int u = 0; u < kNU; ++u) {
      const int pp = p + u * nslots;
      if (pp < k.np) {
        float v[8], o[8];
        unpack8_sel<E>(raw[u], true, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float z = fmaf(v[e], ga[e], be[e]);
          o[e] = ACT ? z * sigmoidf(z) : z;
        }
        store8<E>(y + k.base + (int64_t)pp * C, o);
      }
    }
  }
}

// a + b as its own rounded operation: never contracted with a product that made a or b
__device__ inline float add_alone(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
// o = rn(o) + g, to be rounded once more by the store: what a separate add of g behind the stored o gives
template <class E>
__device__ inline void add_rounded8(float (&o)[8], const Raw8<E> &g) {
  float gv[8];
  unpack8_sel<E>(g, true, gv);
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = add_alone(round_to<E>(o[e]), gv[e]);
}

// backward: t = gamma * dz, xh = (x - mean) * rstd;  per channel and pixel slice: sum t, sum t*xh
template <class E, bool ACT>
__device__ inline void gn_nhwc_terms(const float (&v)[8], const float (&go)[8], const float (&ga)[8],
                                     const float (&be)[8], const float (&mean)[8], const float (&rstd)[8],
                                     const float (&gam)[8], float (&t)[8], float (&xh)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    xh[e] = (v[e] - mean[e]) * rstd[e];
    float dz = go[e];
    if (ACT) dz *= silu_grad(fmaf(v[e], ga[e], be[e]));
    t[e] = gam[e] * dz;
  }
}

// ADD (with APPLY): gsum, a second gradient of x as [B * HW] rows of C channels ldg elements apart (dx's layout when
// ldg = C; a channel slice of a wider gradient otherwise), is loaded next to x and gout and added to the rounded dx (the bits
// of a separate add behind this launch); gsum may be dx itself, each chunk is read before it is written.
template <class E, bool ACT, bool APPLY, bool ADD = false>
__global__ __launch_bounds__(kHT) void gn_nhwc_bwd_kernel(const typename E::storage *__restrict__ x,
                                                          const typename E::storage *__restrict__ gout,
                                                          const typename E::storage *gsum, int64_t ldg,
                                                          const typename E::storage *__restrict__ gamma,
                                                          const float *__restrict__ aff,
                                                          float *__restrict__ part,        // !APPLY: out [B][S][2][C]
                                                          const float *__restrict__ cvec,  // APPLY: [B][2][C] = c1, c2
                                                          typename E::storage *dx, int C, int HW, int cw,
                                                          int tiles, int nslots, int px, int S) {
  static_assert(APPLY || !ADD, "the statistics pass has no second gradient");
  __shared__ __attribute__((aligned(16))) float s_red[APPLY ? 8 : 2 * kHT * 8];
  const NhwcBlock k = nhwc_block(C, HW, cw, tiles, nslots, px, S);
  float ga[8], be[8], mean[8], rstd[8], gam[8], c1[8], c2[8], s1[8], s2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s1[e] = s2[e] = c1[e] = c2[e] = 0.f;
  if (k.active) {
    const float *ab = aff + (int64_t)k.b * 4 * C + (int64_t)k.col * 8;
    ld8f(ab, ga);
    ld8f(ab + C, be);
    ld8f(ab + 2 * C, mean);
    ld8f(ab + 3 * C, rstd);
    unpack8_sel<E>(load8_raw<E>(gamma + (int64_t)k.col * 8), true, gam);
    if (APPLY) {
      ld8f(cvec + (int64_t)k.b * 2 * C + (int64_t)k.col * 8, c1);
      ld8f(cvec + (int64_t)k.b * 2 * C + C + (int64_t)k.col * 8, c2);
    }
    const int64_t gbase = ((int64_t)k.b * HW + (int64_t)k.s * px) * ldg + (int64_t)k.col * 8;
    for (int p = k.slot; p < k.np; p += nslots * kNU) {
      Raw8<E> xr[kNU], gr[kNU], sr[ADD ? kNU : 1];
#pragma unroll
      for (int u = 0; u < kNU; ++u) {
        const int pp = p + u * nslots;
        const int64_t off = k.base + (int64_t)(pp < k.np ? pp : p) * C;
        xr[u] = load8_raw<E>(x + off);
        gr[u] = load8_raw<E>(gout + off);
        if (ADD) sr[u] = load8_raw<E>(gsum + gbase + (int64_t)(pp < k.np ? pp : p) * ldg);
      }
      LORA_AMD_LOADS_ISSUED();
#pragma unroll
      for (int u = 0; u < kNU; ++u) {
        const int pp = p + u * nslots;
        if (pp < k.np) {
          float v[8], go[8], t[8], xh[8];
          unpack8_sel<E>(xr[u], true, v);
          unpack8_sel<E>(gr[u], true, go);
          gn_nhwc_terms<E, ACT>(v, go, ga, be, mean, rstd, gam, t, xh);
          if (APPLY) {
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = rstd[e] * (t[e] - c1[e] - xh[e] * c2[e]);
            if (ADD) add_rounded8<E>(o, sr[u]);
            store8<E>(dx + k.base + (int64_t)pp * C, o);
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              s1[e] += t[e];
              s2[e] = fmaf(t[e], xh[e], s2[e]);
            }
          }
        }
      }
    }
  }
  if (!APPLY) {
    nhwc_slot_reduce(s1, s2, k, cw, nslots, s_red);
    if (k.active && k.slot == 0) {
      float *o = part + ((int64_t)(k.b * S + k.s) * 2) * C + (int64_t)k.col * 8;
      st8f(o, s1);
      st8f(o + C, s2);
    }
  }
}

// cvec[b][0][c] = (sum over the group of s1) / n, cvec[b][1][c] = (sum of s2) / n, expanded per channel
__global__ __launch_bounds__(kHT) void gn_nhwc_bwd_finalize_kernel(const float *__restrict__ part,
                                                                   float *__restrict__ cvec, int C, int HW, int G,
                                                                   int S) {
  __shared__ float s_red[4][2];
  const int b = blockIdx.x / G, g = blockIdx.x - b * G, cpg = C / G;
  float s1 = 0.f, s2 = 0.f;
  for (int i = threadIdx.x; i < S * cpg; i += kHT) {
    const int s = i / cpg, c = g * cpg + (i - s * cpg);
    const float *pp = part + ((int64_t)(b * S + s) * 2) * C + c;
    s1 += pp[0];
    s2 += pp[C];
  }
  block_sum2(s1, s2, s_red);
  const float inv_n = 1.f / ((float)HW * (float)cpg);
  for (int cc = threadIdx.x; cc < cpg; cc += kHT) {
    cvec[(int64_t)b * 2 * C + g * cpg + cc] = s1 * inv_n;
    cvec[(int64_t)b * 2 * C + C + g * cpg + cc] = s2 * inv_n;
  }
}

// ---- resident form: one launch each way on the small maps ----------------------------------------------------------------
// Where a whole (sample, bundle of groups) fits in one workgroup's registers, the statistics, the affine map and the store
// (forward), or both reductions and dx (backward), come from ONE read of each operand.  A bundle is lcm(cpg, 8) adjacent
// channels: a whole number of groups and of 16-byte chunks.  The mapping is the streaming kernels' (thread = pixel slot x
// chunk of the bundle); a thread keeps its NP pixels' chunks raw in registers.  One workgroup owns everything it reduces:
// no workgroup waits for, counts or signals another, and the workspace is not touched.  Every fold runs in a fixed order
// (two launches give the same bits): per-thread channel sums -> LDS -> T / groups threads per group -> wave butterfly.
constexpr int kResMaxChunks = 32;  // chunks per bundle (256 channels)
constexpr int kResMaxGroups = 8;   // groups per bundle = lcm(cpg, 8) / cpg <= 8

// a / b for 0 <= a < 2^22, 1 <= b: one reciprocal and a correction step instead of the ~35-instruction integer division
// (a resident kernel is a latency chain; a dozen divisions in front of its loads were a third of its time)
__device__ inline int res_div(int a, int b) {
  int q = (int)((float)a * fast_rcp((float)b));
  const int r = a - q * b;
  q += r >= b ? 1 : (r < 0 ? -1 : 0);
  return q;
}

struct ResBlock {
  int b, slot, cl, col;
  bool active;
  int64_t base;  // element offset of (b, pixel 0, this thread's chunk)
  int grp[8];    // bundle-local group of each of the chunk's channels
};
__device__ inline ResBlock res_block(int C, int HW, int cpg, int nch, int nslots) {
  ResBlock k;
  const int nb = res_div(C >> 3, nch);
  k.b = res_div(blockIdx.x, nb);
  const int bun = blockIdx.x - k.b * nb;
  k.slot = res_div(threadIdx.x, nch);
  k.cl = threadIdx.x - k.slot * nch;
  k.active = k.slot < nslots;
  k.col = bun * nch + k.cl;
  k.base = (int64_t)k.b * HW * C + (int64_t)k.col * 8;
  int g = res_div(k.cl * 8, cpg), r = k.cl * 8 - g * cpg;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    k.grp[e] = g;
    if (++r == cpg) {
      r = 0;
      ++g;
    }
  }
  return k;
}

template <int T, int NQ>
struct ResLds {
  float red[NQ][T * 8];  // [slot][bundle channel]
  float wp[NQ][T / 32];  // wave (or half-wave) partials, a group's side by side
};

// Sums of s[q] over the bundle's pixel slots and each group's channels -> gs[q][group of the bundle], visible to every
// thread on return.  T / groups threads fold one group: a strided walk over its (slot, channel) entries, a butterfly over
// the wave, then the group's wave partials in order; fin maps the total to what the threads read (mean, rstd).
template <int T, int NQ, class Fin>
__device__ inline void res_group_sum(const float (&s)[NQ][8], const ResBlock &k, int bch, int nslots, int cpg,
                                     ResLds<T, NQ> &l, float (*gs)[kResMaxGroups], Fin fin) {
  const int tid = threadIdx.x;
  __syncthreads();  // the previous fold's readers are done
  if (k.active) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) st8f(l.red[q] + (size_t)tid * 8, s[q]);
  }
  __syncthreads();
  const int ng = res_div(bch, cpg);  // 1, 2, 4 or 8
  const int lg = ng == 1 ? 0 : ng == 2 ? 1 : ng == 4 ? 2 : 3;
  const int L = T >> lg, g = tid >> (__builtin_ctz(T) - lg), lane = tid - g * L;
  const int n = nslots * cpg, dq = res_div(L, cpg), dr = L - dq * cpg;
  int sl = res_div(lane, cpg), c = lane - sl * cpg;
  float a[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) a[q] = 0.f;
#pragma unroll 4
  for (int i = lane; i < n; i += L) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) a[q] += l.red[q][sl * bch + g * cpg + c];
    sl += dq;
    c += dr;
    if (c >= cpg) {
      c -= cpg;
      ++sl;
    }
  }
  const int W = L < 64 ? L : 64;  // T / 8 >= 32
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    if (off < W) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) a[q] += __shfl_xor(a[q], off, 64);
    }
  }
  if ((tid & (W - 1)) == 0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) l.wp[q][tid >> (W == 64 ? 6 : 5)] = a[q];
  }
  __syncthreads();
  if (tid < ng) {
    const int P = L >> (W == 64 ? 6 : 5);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      float t = 0.f;
      for (int i = 0; i < P; ++i) t += l.wp[q][tid * P + i];
      gs[q][tid] = fin(t);
    }
  }
  __syncthreads();
}

template <class E, bool ACT, int T, int NP>
__global__ __launch_bounds__(T) void gn_nhwc_res_fwd_kernel(const typename E::storage *__restrict__ x,
                                                            const typename E::storage *__restrict__ gamma,
                                                            const typename E::storage *__restrict__ beta,
                                                            const float *__restrict__ addend,
                                                            typename E::storage *__restrict__ y, float *__restrict__ aff,
                                                            int C, int HW, int cpg, int nch, int nslots, float eps) {
  __shared__ __attribute__((aligned(16))) ResLds<T, 1> l;
  __shared__ float gs[2][kResMaxGroups];
  const ResBlock k = res_block(C, HW, cpg, nch, nslots);
  Raw8<E> raw[NP];
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    const int p = k.slot + u * nslots;
    raw[u] = load8_raw<E>(x + k.base + (int64_t)(k.active && p < HW ? p : 0) * C);
  }
  float gam[8], bet[8], add[8];
  unpack8_sel<E>(load8_raw<E>(gamma + (int64_t)k.col * 8), true, gam);
  unpack8_sel<E>(load8_raw<E>(beta + (int64_t)k.col * 8), true, bet);
#pragma unroll
  for (int e = 0; e < 8; ++e) add[e] = 0.f;
  if (addend != nullptr) ld8f_sel(addend + (int64_t)k.b * C + (int64_t)k.col * 8, true, add);
  LORA_AMD_LOADS_ISSUED();
  const int bch = nch * 8;
  const float inv_n = 1.f / ((float)HW * (float)cpg);
  float s[1][8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[0][e] = k.slot == 0 ? (float)HW * add[e] : 0.f;  // the addend's share of the channel total
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    float v[8];
    unpack8_sel<E>(raw[u], k.active && k.slot + u * nslots < HW, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) s[0][e] += v[e];
  }
  res_group_sum<T, 1>(s, k, bch, nslots, cpg, l, &gs[0], [=](float t) { return t * inv_n; });  // group means
  float sh[8];  // add - mean: the shift of x in front of the normalisation
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    sh[e] = add[e] - gs[0][k.grp[e]];
    s[0][e] = 0.f;
  }
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    float v[8];
    unpack8_sel<E>(raw[u], true, v);
    if (k.active && k.slot + u * nslots < HW) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = v[e] + sh[e];
        s[0][e] = fmaf(d, d, s[0][e]);
      }
    }
  }
  res_group_sum<T, 1>(s, k, bch, nslots, cpg, l, &gs[1], [=](float t) { return rsqrtf(t * inv_n + eps); });
  float ga[8], bb[8], mn[8], rs[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    rs[e] = gs[1][k.grp[e]];
    ga[e] = gam[e] * rs[e];
    bb[e] = fmaf(sh[e], ga[e], bet[e]);
    mn[e] = -sh[e];
  }
  if (k.slot == 0) {
    float *o = aff + (int64_t)k.b * 4 * C + (int64_t)k.col * 8;
    st8f(o, ga);
    st8f(o + C, bb);
    st8f(o + 2 * C, mn);
    st8f(o + 3 * C, rs);
  }
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    const int p = k.slot + u * nslots;
    if (k.active && p < HW) {
      float v[8], o[8];
      unpack8_sel<E>(raw[u], true, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float z = fmaf(v[e], ga[e], bb[e]);
        o[e] = ACT ? z * sigmoidf(z) : z;
      }
      store8<E>(y + k.base + (int64_t)p * C, o);
    }
  }
}

// ADD: as in gn_nhwc_bwd_kernel (gsum rows ldg elements apart); the gsum chunks are a third raw operand, loaded with the
// other two.
template <class E, bool ACT, int T, int NP, bool ADD = false>
__global__ __launch_bounds__(T) void gn_nhwc_res_bwd_kernel(const typename E::storage *__restrict__ x,
                                                            const typename E::storage *__restrict__ gout,
                                                            const typename E::storage *gsum, int64_t ldg,
                                                            const typename E::storage *__restrict__ gamma,
                                                            const float *__restrict__ aff,
                                                            typename E::storage *dx, int C, int HW, int cpg,
                                                            int nch, int nslots) {
  __shared__ __attribute__((aligned(16))) ResLds<T, 2> l;
  __shared__ float gs[2][kResMaxGroups];
  const ResBlock k = res_block(C, HW, cpg, nch, nslots);
  Raw8<E> xr[NP], gr[NP], sr[ADD ? NP : 1];
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    const int p = k.slot + u * nslots;
    const int pc = k.active && p < HW ? p : 0;
    const int64_t off = k.base + (int64_t)pc * C;
    xr[u] = load8_raw<E>(x + off);
    gr[u] = load8_raw<E>(gout + off);
    if (ADD) sr[u] = load8_raw<E>(gsum + ((int64_t)k.b * HW + pc) * ldg + (int64_t)k.col * 8);
  }
  float ga[8], be[8], mean[8], rstd[8], gam[8];
  const float *ab = aff + (int64_t)k.b * 4 * C + (int64_t)k.col * 8;
  ld8f_sel(ab, true, ga);
  ld8f_sel(ab + C, true, be);
  ld8f_sel(ab + 2 * C, true, mean);
  ld8f_sel(ab + 3 * C, true, rstd);
  unpack8_sel<E>(load8_raw<E>(gamma + (int64_t)k.col * 8), true, gam);
  LORA_AMD_LOADS_ISSUED();
  const int bch = nch * 8;
  float s[2][8];  // sum t, sum t * xh
#pragma unroll
  for (int e = 0; e < 8; ++e) s[0][e] = s[1][e] = 0.f;
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    float v[8], go[8], t[8], xh[8];
    unpack8_sel<E>(xr[u], true, v);
    unpack8_sel<E>(gr[u], true, go);
    gn_nhwc_terms<E, ACT>(v, go, ga, be, mean, rstd, gam, t, xh);
    if (k.active && k.slot + u * nslots < HW) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        s[0][e] += t[e];
        s[1][e] = fmaf(t[e], xh[e], s[1][e]);
      }
    }
  }
  const float inv_n = 1.f / ((float)HW * (float)cpg);
  res_group_sum<T, 2>(s, k, bch, nslots, cpg, l, gs, [=](float t) { return t * inv_n; });
  float c1[8], c2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    c1[e] = gs[0][k.grp[e]];
    c2[e] = gs[1][k.grp[e]];
  }
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    const int p = k.slot + u * nslots;
    if (k.active && p < HW) {
      float v[8], go[8], t[8], xh[8], o[8];
      unpack8_sel<E>(xr[u], true, v);
      unpack8_sel<E>(gr[u], true, go);
      gn_nhwc_terms<E, ACT>(v, go, ga, be, mean, rstd, gam, t, xh);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = rstd[e] * (t[e] - c1[e] - xh[e] * c2[e]);
      if (ADD) add_rounded8<E>(o, sr[u]);
      store8<E>(dx + k.base + (int64_t)p * C, o);
    }
  }
}

// ---- tail of a ResnetBlock2D: both convolution biases and the residual add in one pass ---------------------------------
// out = rn(rn(h + b2) + (bs ? rn(r + bs) : r)) on dense channels_last rows: the three ATen adds behind conv2 and
// conv_shortcut (two strided bias adds, one vectorised add), rounded where they round.  Column-owner mapping as above: a
// thread keeps one 16-byte channel chunk (its bias chunks are loaded once) and walks rows, kNU in flight.
template <class E, bool SB>
__global__ __launch_bounds__(kHT) void resnet_tail_kernel(const typename E::storage *h, int64_t ldh,
                                                          const typename E::storage *r, int64_t ldr,
                                                          const typename E::storage *__restrict__ b2,
                                                          const typename E::storage *__restrict__ bs,
                                                          typename E::storage *out, int64_t ldo, int64_t rows, int c8,
                                                          int cw, int tiles, int nslots, int rpb) {
  const int64_t blk = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x - blk * tiles);
  const int slot = threadIdx.x / cw, cl = threadIdx.x - slot * cw;
  if (slot >= nslots) return;
  const int64_t col = ((int64_t)tile * cw + cl) * 8;
  const int64_t r0 = blk * rpb;
  const int np = (int)min((int64_t)rpb, rows - r0);
  float bv2[8], bvs[8];
  unpack8_sel<E>(load8_raw<E>(b2 + col), true, bv2);
  unpack8_sel<E>(load8_raw<E>(SB ? bs + col : b2 + col), SB, bvs);
  for (int p = slot; p < np; p += nslots * kNU) {
    Raw8<E> hr[kNU], rr[kNU];
#pragma unroll
    for (int u = 0; u < kNU; ++u) {
      const int pp = p + u * nslots;
      const int64_t row = r0 + (pp < np ? pp : p);
      hr[u] = load8_raw<E>(h + row * ldh + col);
      rr[u] = load8_raw<E>(r + row * ldr + col);
    }
    LORA_AMD_LOADS_ISSUED();
#pragma unroll
    for (int u = 0; u < kNU; ++u) {
      const int pp = p + u * nslots;
      if (pp < np) {
        float hv[8], rv[8], o[8];
        unpack8_sel<E>(hr[u], true, hv);
        unpack8_sel<E>(rr[u], true, rv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float a = round_to<E>(hv[e] + bv2[e]);
          const float b = SB ? round_to<E>(rv[e] + bvs[e]) : rv[e];
          o[e] = a + b;
        }
        store8<E>(out + (r0 + pp) * ldo + col, o);
      }
    }
  }
}

// ---- time-embedding addends of every ResnetBlock2D in one launch ------------------------------------------------------
// Each block adds t = time_emb_proj(silu(temb)) + conv1.bias per (sample, channel) in front of its norm2; all of them depend
// on temb and frozen parameters only.  One ragged launch over a table of sites replaces silu + skinny GEMM + bias add +
// widening copy per block.  The kernel is a weight stream (sum N_i rows of K elements, read once): silu(temb) [B][K] sits
// in LDS (rounded to the activation dtype as the separate silu's output is), a wave carries kTembRows weight rows through
// the K loop together (one 16-byte chunk per lane, row and step) against up to BT samples (4 or 8: the products are the
// kernel's VALU work, a batch of 4 must not pay for 8), then a butterfly folds the lanes.  Row g of the launch belongs to the site with row_begin <= g < row_begin + N; a wave's rows may straddle sites.
constexpr int kTembRows = 4;     // weight rows a wave streams together
constexpr int kTembGroups = 2;   // such row groups per wave (amortises the silu prologue)
constexpr int kTembKU = 2;       // 64-chunk K steps in flight
constexpr int kTembMaxSites = kHT;
constexpr int kTembMaxImage = 15360;  // B * K elements: the f32 image is 60 KB of the 64 KB a workgroup may ask for
constexpr int kTembBlockRows = (kHT / kWave) * kTembRows * kTembGroups;

template <class E, int BT>
__global__ __launch_bounds__(kHT) void temb_addends_kernel(const lora_amd_temb_site *__restrict__ sites, int n_sites,
                                                           const typename E::storage *__restrict__ temb,
                                                           float *__restrict__ out, int B, int K) {
  using S = typename E::storage;
  extern __shared__ __attribute__((aligned(32))) unsigned char s_raw[];
  __shared__ int s_begin[kTembMaxSites];
  S *s_x = reinterpret_cast<S *>(s_raw);  // [B][K] = round_E(silu(temb))
  const int c8 = K / 8;
  for (int i = threadIdx.x; i < B * c8; i += kHT) {
    float v[8];
    load8<E>(temb + (int64_t)i * 8, v);
    Chunk8<E> c;
#pragma unroll
    for (int e = 0; e < 8; ++e) c.v[e] = E::from_f(v[e] / (1.f + expf(-v[e])));  // the form ATen's silu evaluates
    *reinterpret_cast<Chunk8<E> *>(s_x + (size_t)i * 8) = c;
  }
  if ((int)threadIdx.x < n_sites) s_begin[threadIdx.x] = gl(sites)[threadIdx.x].row_begin;
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  int si = 0;
  for (int grp = 0; grp < kTembGroups; ++grp) {
    const int64_t g0 = ((int64_t)blockIdx.x * (kHT / kWave) + wave) * (kTembRows * kTembGroups) + grp * kTembRows;
    const S *wp[kTembRows];
    float *op[kTembRows];
    float bias_t[kTembRows], bias_c[kTembRows];
    int n_of[kTembRows];
    bool live[kTembRows], has_c[kTembRows];
#pragma unroll
    for (int j = 0; j < kTembRows; ++j) {
      const int64_t g = g0 + j;
      while (si + 1 < n_sites && g >= s_begin[si + 1]) ++si;
      const lora_amd_temb_site LORA_AMD_AS_GLOBAL *q = gl(sites) + si;
      const int64_t loc = g - s_begin[si];
      n_of[j] = q->N;
      live[j] = loc < n_of[j];  // past the last site's rows: stream row 0 of it, store nothing
      const int64_t r = live[j] ? loc : 0;
      wp[j] = reinterpret_cast<const S *>(q->weight) + r * K;
      bias_t[j] = E::to_f(*gl(reinterpret_cast<const S *>(q->bias) + r));
      has_c[j] = q->conv_bias != nullptr;
      bias_c[j] = has_c[j] ? E::to_f(*gl(reinterpret_cast<const S *>(q->conv_bias) + r)) : 0.f;
      op[j] = out + q->out_offset + r;
    }
    for (int bt = 0; bt < B; bt += BT) {
      float acc[kTembRows][BT];
#pragma unroll
      for (int j = 0; j < kTembRows; ++j)
#pragma unroll
        for (int b = 0; b < BT; ++b) acc[j][b] = 0.f;
      for (int c0 = 0; c0 < c8; c0 += kWave * kTembKU) {
        Raw8<E> wr[kTembKU][kTembRows];
#pragma unroll
        for (int u = 0; u < kTembKU; ++u) {
          const int c = c0 + u * kWave + lane, cs = c < c8 ? c : 0;
#pragma unroll
          for (int j = 0; j < kTembRows; ++j) wr[u][j] = load8_raw<E>(wp[j] + (int64_t)cs * 8);
        }
        LORA_AMD_LOADS_ISSUED();
#pragma unroll
        for (int u = 0; u < kTembKU; ++u) {
          const int c = c0 + u * kWave + lane;
          const bool okc = c < c8;
          const int cs = okc ? c : 0;
          float w[kTembRows][8];
#pragma unroll
          for (int j = 0; j < kTembRows; ++j) unpack8_sel<E>(wr[u][j], okc, w[j]);
#pragma unroll
          for (int b = 0; b < BT; ++b) {
            const int bb = min(bt + b, B - 1);  // samples past B repeat the last one; their sums are not stored
            const Chunk8<E> xc = *reinterpret_cast<const Chunk8<E> *>(s_x + (size_t)bb * K + (size_t)cs * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float xv = E::to_f(xc.v[e]);
#pragma unroll
              for (int j = 0; j < kTembRows; ++j) acc[j][b] = fmaf(w[j][e], xv, acc[j][b]);
            }
          }
        }
      }
      // lanes 0..3 of the wave receive the totals of samples bt + 4 * h + idx4(lane); they apply the two bias adds with
      // the roundings of the sequence this replaces: r1 = rn_E(dot + bias_t), r2 = rn_E(r1 + bias_c), stored as f32
#pragma unroll
      for (int j = 0; j < kTembRows; ++j) {
#pragma unroll
        for (int h = 0; h < BT / 4; ++h) {
          const float tot = wave_sum4(acc[j][4 * h], acc[j][4 * h + 1], acc[j][4 * h + 2], acc[j][4 * h + 3], lane);
          const int b = bt + 4 * h + idx4(lane);
          if (lane < 4 && live[j] && b < B) {
            float r = round_to<E>(tot + bias_t[j]);
            if (has_c[j]) r = round_to<E>(r + bias_c[j]);
            *gl(op[j] + (int64_t)b * n_of[j]) = r;
          }
        }
      }
    }
  }
}

static inline bool aligned_for(const void *p, int dt) { return ((uintptr_t)p % (dt == LORA_AMD_F32 ? 32 : 16)) == 0; }

}  // namespace lora_amd

using namespace lora_amd;

extern "C" size_t lora_amd_groupnorm_workspace(int32_t B, int32_t C, int32_t HW, int32_t groups) {
  const GnGeo q = gn_geo(B, C, HW, groups);
  return q.ok ? (size_t)B * groups * q.S * 2 * sizeof(float) : 0;
}

extern "C" int lora_amd_groupnorm_supported(int32_t B, int32_t C, int32_t HW, int32_t groups) {
  return gn_geo(B, C, HW, groups).ok ? 1 : 0;
}

#define GN_CHECKS(name)                                                                                              \
  const GnGeo q = gn_geo(B, C, HW, groups);                                                                          \
  LORA_AMD_CHECK(q.ok, LORA_AMD_EINVAL, name ": geometry B=%d C=%d HW=%d groups=%d not supported", B, C, HW, groups); \
  LORA_AMD_CHECK(dtype_ok(dtype), LORA_AMD_EINVAL, name ": bad dtype %d", dtype);                                    \
  LORA_AMD_CHECK(workspace_bytes >= lora_amd_groupnorm_workspace(B, C, HW, groups), LORA_AMD_EWORKSPACE,             \
                 name ": workspace %zu < %zu bytes", workspace_bytes, lora_amd_groupnorm_workspace(B, C, HW, groups)); \
  const dim3 grid((unsigned)((int64_t)B * groups * q.S)), block(kHT);                                                \
  hipStream_t st = (hipStream_t)stream;                                                                              \
  float *part = reinterpret_cast<float *>(workspace)

extern "C" int lora_amd_groupnorm_fwd(const void *x, const void *gamma, const void *beta, void *y, float *stats,
                                      void *workspace, size_t workspace_bytes, int32_t B, int32_t C, int32_t HW,
                                      int32_t groups, float eps, int32_t act, int32_t dtype, void *stream) {
  GN_CHECKS("groupnorm_fwd");
  LORA_AMD_CHECK(x && gamma && beta && y && stats && workspace, LORA_AMD_EINVAL, "groupnorm_fwd: null pointer");
  LORA_AMD_CHECK(aligned_for(x, dtype) && aligned_for(y, dtype), LORA_AMD_EINVAL, "groupnorm_fwd: unaligned tensor");
  by_dtype(dtype, [&](auto e) {
    using E = decltype(e);
    using S = typename E::storage;
    hipLaunchKernelGGL((gn_stats_kernel<E>), grid, block, 0, st, (const S *)x, part, groups, q.cpg, HW, q.chunks,
                       q.per_block, q.S);
    by_bool(act != 0, [&](auto a) {
      hipLaunchKernelGGL((gn_apply_kernel<E, decltype(a)::value>), grid, block, 0, st, (const S *)x, (const S *)gamma,
                         (const S *)beta, (S *)y, part, stats, groups, q.cpg, HW, q.chunks, q.per_block, q.S, eps);
    });
  });
  return check_launch("lora_amd_groupnorm_fwd");
}

extern "C" int lora_amd_groupnorm_bwd(const void *x, const void *gout, const void *gamma, const void *beta,
                                      const float *stats, void *dx, void *workspace, size_t workspace_bytes,
                                      int32_t B, int32_t C, int32_t HW, int32_t groups, int32_t act, int32_t dtype,
                                      void *stream) {
  GN_CHECKS("groupnorm_bwd");
  LORA_AMD_CHECK(x && gout && gamma && beta && stats && dx && workspace, LORA_AMD_EINVAL,
                 "groupnorm_bwd: null pointer");
  LORA_AMD_CHECK(aligned_for(x, dtype) && aligned_for(gout, dtype) && aligned_for(dx, dtype), LORA_AMD_EINVAL,
                 "groupnorm_bwd: unaligned tensor");
  by_dtype(dtype, [&](auto e) {
    by_bool(act != 0, [&](auto a) {
      using E = decltype(e);
      using S = typename E::storage;
      constexpr bool A = decltype(a)::value;
      hipLaunchKernelGGL((gn_bwd_stats_kernel<E, A>), grid, block, 0, st, (const S *)x, (const S *)gout,
                         (const S *)gamma, (const S *)beta, stats, part, groups, q.cpg, HW, q.chunks, q.per_block,
                         q.S);
      hipLaunchKernelGGL((gn_bwd_apply_kernel<E, A>), grid, block, 0, st, (const S *)x, (const S *)gout,
                         (const S *)gamma, (const S *)beta, stats, part, (S *)dx, groups, q.cpg, HW, q.chunks,
                         q.per_block, q.S);
    });
  });
  return check_launch("lora_amd_groupnorm_bwd");
}

#define GEGLU_CHECKS(name)                                                                                      \
  LORA_AMD_CHECK(M >= 0 && inner > 0 && inner % 8 == 0, LORA_AMD_EINVAL, name ": bad shape M=%lld inner=%d",     \
                 (long long)M, inner);                                                                          \
  LORA_AMD_CHECK(dtype_ok(dtype), LORA_AMD_EINVAL, name ": bad dtype %d", dtype);                                \
  if (M == 0) return LORA_AMD_OK;                                                                               \
  hipStream_t st = (hipStream_t)stream;                                                                         \
  const int c8 = inner / 8;                                                                                     \
  const int64_t total = M * c8;                                                                                 \
  LORA_AMD_CHECK(total < (1ll << 31), LORA_AMD_EINVAL, name ": M * inner / 8 = %lld exceeds 2^31", (long long)total)

extern "C" int lora_amd_geglu_fwd(const void *y, int64_t ldy, void *out, int64_t ldo, int64_t M, int32_t inner,
                                  int32_t dtype, void *stream) {
  GEGLU_CHECKS("geglu_fwd");
  LORA_AMD_CHECK(y && out, LORA_AMD_EINVAL, "geglu_fwd: null pointer");
  LORA_AMD_CHECK(ldy >= 2 * (int64_t)inner && ldo >= inner && ldy % 8 == 0 && ldo % 8 == 0 && aligned_for(y, dtype) &&
                     aligned_for(out, dtype),
                 LORA_AMD_EINVAL, "geglu_fwd: rows must be 16-byte aligned (ldy=%lld ldo=%lld)", (long long)ldy,
                 (long long)ldo);
  const dim3 grid((unsigned)((total + kHT * kHU - 1) / (kHT * kHU))), block(kHT);
  by_dtype(dtype, [&](auto e) {
    using S = typename decltype(e)::storage;
    hipLaunchKernelGGL((geglu_fwd_kernel<decltype(e)>), grid, block, 0, st, (const S *)y, ldy, (S *)out, ldo, M, c8);
  });
  return check_launch("lora_amd_geglu_fwd");
}

extern "C" int lora_amd_geglu_bwd(const void *y, int64_t ldy, const void *gout, int64_t ldg, void *gy, int64_t ldgy,
                                  int64_t M, int32_t inner, int32_t dtype, void *stream) {
  GEGLU_CHECKS("geglu_bwd");
  LORA_AMD_CHECK(y && gout && gy, LORA_AMD_EINVAL, "geglu_bwd: null pointer");
  LORA_AMD_CHECK(ldy >= 2 * (int64_t)inner && ldgy >= 2 * (int64_t)inner && ldg >= inner && ldy % 8 == 0 &&
                     ldgy % 8 == 0 && ldg % 8 == 0 && aligned_for(y, dtype) && aligned_for(gout, dtype) &&
                     aligned_for(gy, dtype),
                 LORA_AMD_EINVAL, "geglu_bwd: rows must be 16-byte aligned");
  const dim3 grid((unsigned)((total + kHT * 2 - 1) / (kHT * 2))), block(kHT);
  by_dtype(dtype, [&](auto e) {
    using S = typename decltype(e)::storage;
    hipLaunchKernelGGL((geglu_bwd_kernel<decltype(e)>), grid, block, 0, st, (const S *)y, ldy, (const S *)gout, ldg, (S *)gy,
                       ldgy, M, c8);
  });
  return check_launch("lora_amd_geglu_bwd");
}

extern "C" int lora_amd_layernorm_supported(int32_t K) { return K > 0 && K % 8 == 0 && ln_logL(K / 8) >= 0 ? 1 : 0; }

#define LN_CHECKS(name)                                                                                          \
  LORA_AMD_CHECK(M >= 0 && lora_amd_layernorm_supported(K), LORA_AMD_EINVAL, name ": bad shape M=%lld K=%d",      \
                 (long long)M, K);                                                                               \
  LORA_AMD_CHECK(dtype_ok(dtype), LORA_AMD_EINVAL, name ": bad dtype %d", dtype);                                 \
  if (M == 0) return LORA_AMD_OK;                                                                                \
  hipStream_t st = (hipStream_t)stream;                                                                          \
  const int c8 = K / 8, logL = ln_logL(c8);                                                                      \
  const int rows_per_block = kHT >> logL;                                                                        \
  const dim3 grid((unsigned)((M + rows_per_block - 1) / rows_per_block)), block(kHT)

extern "C" int lora_amd_layernorm_fwd(const void *x, const void *res, const void *gamma, const void *beta, void *sum_out,
                                      void *y, float *stats, int64_t M, int32_t K, float eps, int32_t dtype,
                                      void *stream) {
  LN_CHECKS("layernorm_fwd");
  LORA_AMD_CHECK(x && gamma && beta && y && stats, LORA_AMD_EINVAL, "layernorm_fwd: null pointer");
  LORA_AMD_CHECK((res == nullptr) == (sum_out == nullptr), LORA_AMD_EINVAL,
                 "layernorm_fwd: res and sum_out go together");
  LORA_AMD_CHECK(aligned_for(x, dtype) && aligned_for(y, dtype) && aligned_for(gamma, dtype) && aligned_for(beta, dtype) &&
                     aligned_for(res, dtype) && aligned_for(sum_out, dtype),
                 LORA_AMD_EINVAL, "layernorm_fwd: unaligned tensor");
  const bool add = res != nullptr;
  by_dtype(dtype, [&](auto e) {
    by_bool(add, [&](auto a) {  // without the residual, res and sum_out are null
      using S = typename decltype(e)::storage;
      hipLaunchKernelGGL((ln_fwd_kernel<decltype(e), decltype(a)::value>), grid, block, 0, st, (const S *)x, (const S *)res,
                         (const S *)gamma, (const S *)beta, (S *)sum_out, (S *)y, stats, M, c8, logL, eps);
    });
  });
  return check_launch("lora_amd_layernorm_fwd");
}

extern "C" int lora_amd_layernorm_bwd(const void *x, const void *gout, const void *gsum, const void *gamma,
                                      const float *stats, void *dx, int64_t M, int32_t K, int32_t dtype, void *stream) {
  LN_CHECKS("layernorm_bwd");
  LORA_AMD_CHECK(x && gout && gamma && stats && dx, LORA_AMD_EINVAL, "layernorm_bwd: null pointer");
  LORA_AMD_CHECK(aligned_for(x, dtype) && aligned_for(gout, dtype) && aligned_for(dx, dtype) && aligned_for(gamma, dtype) &&
                     aligned_for(gsum, dtype),
                 LORA_AMD_EINVAL, "layernorm_bwd: unaligned tensor");
  by_dtype(dtype, [&](auto e) {
    by_bool(gsum != nullptr, [&](auto a) {
      using S = typename decltype(e)::storage;
      hipLaunchKernelGGL((ln_bwd_kernel<decltype(e), decltype(a)::value>), grid, block, 0, st, (const S *)x, (const S *)gout,
                         (const S *)gsum, (const S *)gamma, stats, (S *)dx, M, c8, logL);
    });
  });
  return check_launch("lora_amd_layernorm_bwd");
}

// ---- channels_last GroupNorm entry points ----------------------------------------------------------------------
static size_t gn_nhwc_part_floats(const GnNhwcGeo &q, int B, int C) { return (size_t)B * q.S * 2 * C; }

extern "C" size_t lora_amd_groupnorm_nhwc_workspace(int32_t B, int32_t C, int32_t HW, int32_t groups) {
  const GnNhwcGeo q = gn_nhwc_geo(B, C, HW, groups);
  return q.ok ? (gn_nhwc_part_floats(q, B, C) + (size_t)B * 2 * C) * sizeof(float) : 0;
}

// Resident route (gn_nhwc_res_*_kernel).  The (workgroup size, pixels per thread) forms that exist, in the order tried.
// A thread's raw registers are NP chunks of 4 (16-bit) or 8 (f32) dwords, twice that backward; they must leave room for
// the working set (five per-channel vectors, the sums, one pixel's terms) inside the 256 registers a lane of a 512-thread
// workgroup has.  The bounds are the compiler's verdict, not an estimate: profiles/gn_resident_resources.txt lists every
// instantiation with scratch 0.  Forms that spilled when tried (1024 threads x 8 or 16 pixels forward, 512 x 16 16-bit
// backward) do not exist; their geometries stay on the streaming kernels.
struct GnResForm {
  int T, NP;
};
constexpr GnResForm kResForms[] = {{256, 2}, {512, 4}, {512, 8}, {512, 16}};
constexpr int kResNForms = (int)(sizeof(kResForms) / sizeof(kResForms[0]));
constexpr int res_raw_regs(int form, int esize, bool bwd) { return kResForms[form].NP * esize * 2 * (bwd ? 2 : 1); }
constexpr bool res_form_fits(int form, int esize, bool bwd) { return res_raw_regs(form, esize, bwd) <= (bwd ? 64 : 128); }
// the backward with gsum keeps a third raw operand; the same working set has to fit beside it
constexpr bool res_form_fits_add(int form, int esize) {
  return res_form_fits(form, esize, true) && res_raw_regs(form, esize, true) * 3 / 2 <= 96;
}

struct GnResPlan {
  int form, cpg, nch, nslots;  // form < 0: no resident form holds this geometry
  unsigned grid;
};
static GnResPlan gn_nhwc_res_plan(int B, int C, int HW, int G, int dtype, bool bwd, bool add = false) {
  GnResPlan p{-1, 0, 0, 0, 0};
  p.cpg = C / G;
  int bch = p.cpg;
  while (bch % 8) bch += p.cpg;  // lcm(cpg, 8)
  p.nch = bch / 8;
  if (p.nch > kResMaxChunks || (int64_t)B * (C / bch) >= (1 << 22)) return p;  // res_div's range
  p.grid = (unsigned)(B * (C / bch));
  for (int f = 0; f < kResNForms; ++f) {
    const int nslots = std::min(kResForms[f].T / p.nch, HW);
    const bool fits = add ? res_form_fits_add(f, dtype_size(dtype)) : res_form_fits(f, dtype_size(dtype), bwd);
    if (!fits || (int64_t)nslots * kResForms[f].NP < HW) continue;
    p.form = f;
    p.nslots = nslots;
    break;
  }
  return p;
}

static std::atomic<int> g_gn_resident{1};

// The measured half of the rule (profiles/gn_resident_kbench.txt, graph-timed per geometry of the flagship step): the
// resident launch beat the three streaming launches at every geometry a form holds, so capacity alone decides.
static bool gn_nhwc_res_faster(int B, int C, int HW, int G, int dtype, bool bwd) {
  (void)B, (void)C, (void)HW, (void)G, (void)dtype, (void)bwd;
  return true;
}

// 1 = resident, 0 = streaming; a pure function of the geometry (a captured graph replays the same kernels everywhere)
static int gn_nhwc_route(int B, int C, int HW, int G, int dtype, int dir, bool add = false) {
  if (!g_gn_resident.load(std::memory_order_relaxed)) return 0;
  return gn_nhwc_res_plan(B, C, HW, G, dtype, dir != 0, add).form >= 0 && gn_nhwc_res_faster(B, C, HW, G, dtype, dir != 0) ? 1 : 0;
}

extern "C" int lora_amd_groupnorm_nhwc_resident(int32_t enable) {
  const int prev = g_gn_resident.load(std::memory_order_relaxed);
  if (enable >= 0) g_gn_resident.store(enable ? 1 : 0, std::memory_order_relaxed);
  return prev;
}

extern "C" int lora_amd_groupnorm_nhwc_route(int32_t B, int32_t C, int32_t HW, int32_t groups, int32_t dtype,
                                             int32_t backward, int32_t add) {
  LORA_AMD_CHECK(gn_nhwc_geo(B, C, HW, groups).ok, LORA_AMD_EINVAL,
                 "groupnorm_nhwc_route: geometry B=%d C=%d HW=%d groups=%d not supported", B, C, HW, groups);
  LORA_AMD_CHECK(dtype_ok(dtype), LORA_AMD_EINVAL, "groupnorm_nhwc_route: bad dtype %d", dtype);
  LORA_AMD_CHECK(!add || backward, LORA_AMD_EINVAL, "groupnorm_nhwc_route: only the backward takes a gradient addend");
  return gn_nhwc_route(B, C, HW, groups, dtype, backward, add != 0);
}

// f(int_c<form>) for the plan's form
template <class F>
static void res_by_form(int form, F &&f) {
  by_int<0, 1, 2, 3>(form, f);
  static_assert(kResNForms == 4, "res_by_form lists every form");
}

#define GN_NHWC_CHECKS(name)                                                                                          \
  const GnNhwcGeo q = gn_nhwc_geo(B, C, HW, groups);                                                                  \
  LORA_AMD_CHECK(q.ok, LORA_AMD_EINVAL, name ": geometry B=%d C=%d HW=%d groups=%d not supported", B, C, HW, groups); \
  LORA_AMD_CHECK(dtype_ok(dtype), LORA_AMD_EINVAL, name ": bad dtype %d", dtype);                                     \
  LORA_AMD_CHECK(workspace_bytes >= lora_amd_groupnorm_nhwc_workspace(B, C, HW, groups), LORA_AMD_EWORKSPACE,         \
                 name ": workspace %zu bytes too small", workspace_bytes);                                            \
  const dim3 grid((unsigned)((int64_t)B * q.S * q.tiles)), gridg((unsigned)(B * groups)), block(kHT);                 \
  hipStream_t st = (hipStream_t)stream;                                                                               \
  float *part = reinterpret_cast<float *>(workspace);                                                                 \
  float *cvec = part + gn_nhwc_part_floats(q, B, C);                                                                  \
  (void)cvec

extern "C" int lora_amd_groupnorm_nhwc_fwd(const void *x, const void *gamma, const void *beta, const float *addend,
                                           void *y, float *aff, void *workspace, size_t workspace_bytes, int32_t B, int32_t C, int32_t HW,
                                           int32_t groups, float eps, int32_t act, int32_t dtype, void *stream) {
  GN_NHWC_CHECKS("groupnorm_nhwc_fwd");
  LORA_AMD_CHECK(x && gamma && beta && y && aff && workspace, LORA_AMD_EINVAL, "groupnorm_nhwc_fwd: null pointer");
  LORA_AMD_CHECK(aligned_for(x, dtype) && aligned_for(y, dtype) && ((uintptr_t)aff % 32) == 0, LORA_AMD_EINVAL,
                 "groupnorm_nhwc_fwd: unaligned tensor");
  if (gn_nhwc_route(B, C, HW, groups, dtype, 0)) {
    const GnResPlan p = gn_nhwc_res_plan(B, C, HW, groups, dtype, false);
    by_dtype(dtype, [&](auto e) {
      by_bool(act != 0, [&](auto a) {
        res_by_form(p.form, [&](auto f) {
          using E = decltype(e);
          using S = typename E::storage;
          constexpr int F = decltype(f)::value;
          if constexpr (res_form_fits(F, (int)sizeof(S), false))
            hipLaunchKernelGGL((gn_nhwc_res_fwd_kernel<E, decltype(a)::value, kResForms[F].T, kResForms[F].NP>), dim3(p.grid),
                               dim3(kResForms[F].T), 0, st, (const S *)x, (const S *)gamma, (const S *)beta, addend, (S *)y,
                               aff, C, HW, p.cpg, p.nch, p.nslots, eps);
        });
      });
    });
    return check_launch("lora_amd_groupnorm_nhwc_fwd");
  }
  by_dtype(dtype, [&](auto e) {
    using E = decltype(e);
    using S = typename E::storage;
    hipLaunchKernelGGL((gn_nhwc_stats_kernel<E>), grid, block, 0, st, (const S *)x, part, C, HW, q.cw, q.tiles,
                       q.nslots, q.px, q.S);
    hipLaunchKernelGGL((gn_nhwc_finalize_kernel<E>), gridg, block, 0, st, part, (const S *)gamma, (const S *)beta,
                       addend, aff, C, HW, groups, q.px, q.S, eps);
    by_bool(act != 0, [&](auto a) {
      hipLaunchKernelGGL((gn_nhwc_apply_kernel<E, decltype(a)::value>), grid, block, 0, st, (const S *)x, aff, (S *)y, C, HW,
                         q.cw, q.tiles, q.nslots, q.px, q.S);
    });
  });
  return check_launch("lora_amd_groupnorm_nhwc_fwd");
}

extern "C" int lora_amd_groupnorm_nhwc_bwd(const void *x, const void *gout, const void *gsum, int64_t ld_gsum,
                                           const void *gamma, const float *aff, void *dx, void *workspace,
                                           size_t workspace_bytes, int32_t B, int32_t C, int32_t HW, int32_t groups,
                                           int32_t act, int32_t dtype, void *stream) {
  GN_NHWC_CHECKS("groupnorm_nhwc_bwd");
  LORA_AMD_CHECK(x && gout && gamma && aff && dx && workspace, LORA_AMD_EINVAL, "groupnorm_nhwc_bwd: null pointer");
  LORA_AMD_CHECK(aligned_for(x, dtype) && aligned_for(gout, dtype) && aligned_for(dx, dtype) &&
                     aligned_for(gamma, dtype) && aligned_for(gsum, dtype) && ((uintptr_t)aff % 32) == 0,
                 LORA_AMD_EINVAL, "groupnorm_nhwc_bwd: unaligned tensor");
  const bool add = gsum != nullptr;
  LORA_AMD_CHECK(!add || (ld_gsum >= C && ld_gsum % 8 == 0), LORA_AMD_EINVAL,
                 "groupnorm_nhwc_bwd: gsum row stride %lld (a multiple of 8, at least C = %d)", (long long)ld_gsum, C);
  if (gn_nhwc_route(B, C, HW, groups, dtype, 1, add)) {
    const GnResPlan p = gn_nhwc_res_plan(B, C, HW, groups, dtype, true, add);
    by_dtype(dtype, [&](auto e) {
      by_bool(act != 0, [&](auto a) {
        by_bool(add, [&](auto ad) {
          res_by_form(p.form, [&](auto f) {
            using E = decltype(e);
            using S = typename E::storage;
            constexpr int F = decltype(f)::value;
            constexpr bool AD = decltype(ad)::value;
            if constexpr (AD ? res_form_fits_add(F, (int)sizeof(S)) : res_form_fits(F, (int)sizeof(S), true))
              hipLaunchKernelGGL((gn_nhwc_res_bwd_kernel<E, decltype(a)::value, kResForms[F].T, kResForms[F].NP, AD>),
                                 dim3(p.grid), dim3(kResForms[F].T), 0, st, (const S *)x, (const S *)gout, (const S *)gsum,
                                 ld_gsum, (const S *)gamma, aff, (S *)dx, C, HW, p.cpg, p.nch, p.nslots);
          });
        });
      });
    });
    return check_launch("lora_amd_groupnorm_nhwc_bwd");
  }
  by_dtype(dtype, [&](auto e) {
    by_bool(act != 0, [&](auto a) {
      using E = decltype(e);
      using S = typename E::storage;
      constexpr bool A = decltype(a)::value;
      hipLaunchKernelGGL((gn_nhwc_bwd_kernel<E, A, false>), grid, block, 0, st, (const S *)x, (const S *)gout,
                         (const S *)nullptr, (int64_t)0, (const S *)gamma, aff, part, (const float *)nullptr, (S *)nullptr, C, HW, q.cw,
                         q.tiles, q.nslots, q.px, q.S);
      hipLaunchKernelGGL(gn_nhwc_bwd_finalize_kernel, gridg, block, 0, st, part, cvec, C, HW, groups, q.S);
      by_bool(add, [&](auto ad) {
        hipLaunchKernelGGL((gn_nhwc_bwd_kernel<E, A, true, decltype(ad)::value>), grid, block, 0, st, (const S *)x,
                           (const S *)gout, (const S *)gsum, ld_gsum, (const S *)gamma, aff, (float *)nullptr, cvec, (S *)dx, C, HW,
                           q.cw, q.tiles, q.nslots, q.px, q.S);
      });
    });
  });
  return check_launch("lora_amd_groupnorm_nhwc_bwd");
}

// ---- ResnetBlock2D tail entry point ------------------------------------------------------------------------------------
extern "C" int lora_amd_resnet_tail(const void *h, int64_t ldh, const void *r, int64_t ldr, const void *b2, const void *bs,
                                    void *out, int64_t ldo, int64_t rows, int32_t C, int32_t dtype, void *stream) {
  LORA_AMD_CHECK(dtype_ok(dtype), LORA_AMD_EINVAL, "resnet_tail: bad dtype %d", dtype);
  LORA_AMD_CHECK(rows >= 0 && C > 0 && C % 8 == 0 && ldh >= C && ldr >= C && ldo >= C && ldh % 8 == 0 && ldr % 8 == 0 &&
                     ldo % 8 == 0,
                 LORA_AMD_EINVAL, "resnet_tail: bad shape rows=%lld C=%d strides %lld / %lld / %lld", (long long)rows, C,
                 (long long)ldh, (long long)ldr, (long long)ldo);
  if (rows == 0) return LORA_AMD_OK;
  LORA_AMD_CHECK(h && r && b2 && out, LORA_AMD_EINVAL, "resnet_tail: null pointer");
  LORA_AMD_CHECK(aligned_for(h, dtype) && aligned_for(r, dtype) && aligned_for(out, dtype) && aligned_for(b2, dtype) &&
                     aligned_for(bs, dtype),
                 LORA_AMD_EINVAL, "resnet_tail: unaligned tensor");
  const GnNhwcGeo q = gn_nhwc_geo(1, C, 1, 1);  // the column-owner split of C: cw chunks x nslots rows per workgroup
  // rows per workgroup: ~1024 workgroups on the large maps, at least kNU rows per slot
  int64_t rpb = std::max<int64_t>((int64_t)kNU * q.nslots, rows * q.tiles / 1024);
  rpb = std::min<int64_t>(rpb, rows);
  const int64_t nblk = (rows + rpb - 1) / rpb;
  LORA_AMD_CHECK(nblk * q.tiles < (1ll << 31), LORA_AMD_EINVAL, "resnet_tail: %lld rows exceed the grid", (long long)rows);
  const dim3 grid((unsigned)(nblk * q.tiles)), block(kHT);
  by_dtype(dtype, [&](auto e) {
    by_bool(bs != nullptr, [&](auto sb) {
      using S = typename decltype(e)::storage;
      hipLaunchKernelGGL((resnet_tail_kernel<decltype(e), decltype(sb)::value>), grid, block, 0, (hipStream_t)stream,
                         (const S *)h, ldh, (const S *)r, ldr, (const S *)b2, (const S *)bs, (S *)out, ldo, rows, q.c8, q.cw,
                         q.tiles, q.nslots, (int)rpb);
    });
  });
  return check_launch("lora_amd_resnet_tail");
}

// ---- time-embedding addends entry points ------------------------------------------------------------------------------
extern "C" int lora_amd_temb_addends_supported(int32_t B, int32_t K, int32_t dtype) {
  return B > 0 && K > 0 && K % 8 == 0 && (int64_t)B * K <= kTembMaxImage && dtype_ok(dtype) ? 1 : 0;
}

extern "C" int lora_amd_temb_addends(const lora_amd_temb_site *sites_dev, int32_t n_sites, int64_t total_rows,
                                     const void *temb, float *out, int32_t B, int32_t K, int32_t dtype, void *stream) {
  LORA_AMD_CHECK(lora_amd_temb_addends_supported(B, K, dtype), LORA_AMD_EINVAL,
                 "temb_addends: B=%d K=%d dtype=%d not supported (K %% 8 == 0, B * K <= %d)", B, K, dtype, kTembMaxImage);
  LORA_AMD_CHECK(n_sites >= 0 && n_sites <= kTembMaxSites && total_rows >= 0 && total_rows < (1ll << 31),
                 LORA_AMD_EINVAL, "temb_addends: %d sites / %lld rows (at most %d sites)", n_sites, (long long)total_rows,
                 kTembMaxSites);
  if (n_sites == 0 || total_rows == 0) return LORA_AMD_OK;
  LORA_AMD_CHECK(sites_dev && temb && out, LORA_AMD_EINVAL, "temb_addends: null pointer");
  LORA_AMD_CHECK(aligned_for(temb, dtype) && ((uintptr_t)out % 4) == 0 && ((uintptr_t)sites_dev % 8) == 0, LORA_AMD_EINVAL,
                 "temb_addends: unaligned tensor");
  const dim3 grid((unsigned)((total_rows + kTembBlockRows - 1) / kTembBlockRows)), block(kHT);
  const size_t lds = (size_t)B * K * dtype_size(dtype);
  by_dtype(dtype, [&](auto e) {
    using S = typename decltype(e)::storage;
    by_int<4, 8>(B <= 4 ? 4 : 8, [&](auto bt) {  // samples per pass over the weights
      hipLaunchKernelGGL((temb_addends_kernel<decltype(e), decltype(bt)::value>), grid, block, lds, (hipStream_t)stream,
                         sites_dev, n_sites, (const S *)temb, out, B, K);
    });
  });
  return check_launch("lora_amd_temb_addends");
}
