// Backward of softmax(scale Q K^T) V for SHORT key axes (1 <= Sk <= 80: the 77 text tokens of the cross-attention layers).
//
// The library's flash backward parallelises dK / dV over key blocks: with 77 keys that is two key blocks x (batch x head)
// workgroups on 256 CUs, each walking every query serially (69 us per call for 4 GFLOP and 50 MB).  Here the whole key axis
// is ONE tile, so there is no online softmax, no log-sum-exp and no saved output: the row statistics are exact reductions
// over the 80 scores a query owns, and delta_i = sum_j P_ij dP_ij comes out of the same registers as P.
//
//   P  = softmax(scale Q K^T)      dP = dO V^T        delta = rowsum(P o dP)       dS = P o (dP - delta)
//   dQ = scale dS K                dK = scale dS^T Q  dV    = P^T dO
//
// One workgroup = 256 threads = 4 waves walks a run of consecutive 64-query blocks of one (batch, head); wave w owns queries
// 16 w .. 16 w + 15 of a block.  K and V [80][D] (rows >= Sk zero) and K^T [D][80] are staged in LDS once per workgroup; the
// block's Q and dO rows are staged per block (the next block's rows are already in flight in registers).  All five products are
// v_mfma_f32_16x16x32 with the fragment conventions of mfma16.hpp:
//
//   S^T, dP^T  A = K / V rows (LDS), B = Q / dO rows (LDS), k = head dim: lane l holds query l & 15, keys 16 t + 4 (l >> 4) + reg,
//              t = 0..4, i.e. 20 scores; max / sum / delta are in-lane reductions plus exchanges with lanes l ^ 16, l ^ 32 (f32)
//   dQ^T       A = K^T rows (LDS), B = dS rows (bf16, the wave's own 16 rows of an LDS image [64][80]), k = key: lane l holds
//              query l & 15 and 4 consecutive head-dim columns, stored as 8 bytes
//   dK, dV     A = dS^T / P^T rows (bf16 LDS images [80][64], written transposed from the score registers), B = the block's Q / dO
//              columns gathered from their row images by 2-byte LDS reads, k = query; f32 accumulators live in registers over the
//              whole run, the head-dim tiles dealt round the four waves
//
// P and dS are rounded to 16 bits once (where they become matrix operands), everything else is f32.  A trailing half k-step
// (D % 32 == 16; keys 64..79) is fed zeros in the upper two lane groups.  Each workgroup stores ONE f32 slab [2][80][D] of dK / dV
// partials; a second launch sums a (batch, head)'s slabs in slab order and writes dK / dV: no atomics, no workgroup ever waits for
// another, same bits on every run.  Nothing past row Sk of k / v or row Sq of q / dO / dq is read or written.
#include <math.h>

#include "common.hpp"
#include "mfma16.hpp"

namespace lora_amd {
namespace {

constexpr int kKeys = 80;      // key rows of every LDS image (5 tiles of 16)
constexpr int kKeyTiles = 5;
constexpr int kBlockQ = 64;    // queries per block: 16 per wave
constexpr int kLdKey = 88;     // row stride of the key-contiguous images (K^T [D][80], dS [64][80]): 176 bytes
constexpr int kLdQry = 72;     // row stride of the query-contiguous images (P^T, dS^T [80][64]): 144 bytes
constexpr int kThreads = 256;
constexpr int kMinRun = 4;          // blocks behind one staging of K / V and one slab (fewer: the slabs outweigh the rows)
constexpr int kTargetGroups = 256;  // one workgroup per CU: the LDS footprint (87 KB at D = 64, 156 KB at D = 160) allows no second

template <class S>
struct AttnShortArgs {
  const S *q, *k, *v, *go;
  S *dq;
  float *ws;
  int64_t qs[3], ks[3], vs[3], gs[3], dqs[3];  // (batch, head, row) strides in elements; the last dimension is dense
  int Sq, Sk, H, run, slabs, need_kv;
  float scale;
};

template <class S>
struct AttnShortFoldArgs {
  const float *ws;
  S *dk, *dv;
  int64_t dks[3], dvs[3];
  int Sk, H, slabs;
};

// 16 bytes of row `row`, elements col .. col + 7 of an LDS image as an MFMA operand; `dead` lanes (the upper half of a trailing
// half k-step) read a valid address and get zeros
template <class E>
__device__ __forceinline__ typename FmMfma<E>::frag lds_frag(const typename E::storage *img, int row, int ld, int col, bool dead) {
  mu32x4 v = *reinterpret_cast<const mu32x4 *>(img + row * ld + (dead ? 0 : col));
  if (dead) v = mu32x4{0u, 0u, 0u, 0u};
  return fm_frag<E>(v);
}

// B operand whose k axis runs down the ROWS of a row-major image: elements img[row0 + e][col], e = 0..7 (2-byte reads)
template <class E>
__device__ __forceinline__ typename FmMfma<E>::frag lds_frag_col(const typename E::storage *img, int row0, int ld, int col) {
  union { typename FmMfma<E>::frag f; typename E::storage s[8]; } u;
#pragma unroll
  for (int e = 0; e < 8; ++e) u.s[e] = img[(row0 + e) * ld + col];
  return u.f;
}

template <class E, int D>
__global__ __launch_bounds__(kThreads) void attn_short_bwd_kernel(const AttnShortArgs<typename E::storage> a) {
  using S = typename E::storage;
  using frag = typename FmMfma<E>::frag;
  constexpr int LD = D + 8;                 // row stride of the head-dim-contiguous images
  constexpr int CH = D / 8;                 // 16-byte chunks per row
  constexpr int KSD = (D + 31) / 32;        // k-steps over the head dimension
  constexpr bool HALF_D = D % 32 == 16;     // the last of them is a half step
  constexpr int KSK = 3;                    // k-steps over the 80 keys: 32 + 32 + 16
  constexpr int NDT = D / 16;               // head-dim tiles of dQ / dK / dV
  constexpr int TPW = (NDT + 3) / 4;        // dK / dV head-dim tiles per wave
  constexpr int NLD = (kBlockQ * CH + kThreads - 1) / kThreads;  // 16-byte chunks of a block's Q (and dO) per thread

  __shared__ __attribute__((aligned(16))) S Ks[kKeys * LD];
  __shared__ __attribute__((aligned(16))) S Vs[kKeys * LD];
  __shared__ __attribute__((aligned(16))) S Kt[D * kLdKey];
  __shared__ __attribute__((aligned(16))) S Qs[kBlockQ * LD];
  __shared__ __attribute__((aligned(16))) S Gs[kBlockQ * LD];
  __shared__ __attribute__((aligned(16))) S dSq[kBlockQ * kLdKey];
  __shared__ __attribute__((aligned(16))) S Pt[kKeys * kLdQry];
  __shared__ __attribute__((aligned(16))) S dSt[kKeys * kLdQry];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  const int bh = blockIdx.x / a.slabs, slab = blockIdx.x % a.slabs;
  const int b = bh / a.H, h = bh % a.H;
  const int Sq = a.Sq, Sk = a.Sk;
  const int nblk = (Sq + kBlockQ - 1) / kBlockQ;
  const int blk0 = slab * a.run, blk1 = min(nblk, blk0 + a.run);
  const S *qb = a.q + b * a.qs[0] + h * a.qs[1];
  const S *gb = a.go + b * a.gs[0] + h * a.gs[1];
  const S *kb = a.k + b * a.ks[0] + h * a.ks[1];
  const S *vb = a.v + b * a.vs[0] + h * a.vs[1];
  S *dqb = a.dq + b * a.dqs[0] + h * a.dqs[1];

  // the block's Q / dO rows travel through registers: issued one block ahead, written to LDS at the top of the block
  mu32x4 rq[NLD], rg[NLD];
  auto fetch = [&](int blk) {
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      const int i = tid + j * kThreads, row = i / CH, ch = i % CH;
      const int qi = blk * kBlockQ + row;
      const bool ok = row < kBlockQ && qi < Sq;
      const int64_t qc = ok ? qi : Sq - 1;  // a valid row: the value is dropped
      const mu32x4 x = *gl(reinterpret_cast<const mu32x4 *>(qb + qc * a.qs[2] + ch * 8));
      const mu32x4 y = *gl(reinterpret_cast<const mu32x4 *>(gb + qc * a.gs[2] + ch * 8));
      rq[j] = ok ? x : mu32x4{0u, 0u, 0u, 0u};
      rg[j] = ok ? y : mu32x4{0u, 0u, 0u, 0u};
    }
  };
  if (blk0 < blk1) fetch(blk0);  // in flight while K / V are staged

  // ---- K, V and K^T of this (batch, head): rows >= Sk are zeros and never read from memory (the load takes row Sk - 1 and
  // its value is dropped: branch-free, so every load of the loop is in flight before the first LDS write)
  constexpr int NKV = (kKeys * CH + kThreads - 1) / kThreads;
  mu32x4 rk[NKV], rv[NKV];
#pragma unroll
  for (int j = 0; j < NKV; ++j) {
    const int i = tid + j * kThreads, row = i / CH, ch = i % CH;
    const bool ok = row < Sk;
    const int rc = ok ? row : Sk - 1;
    const mu32x4 x = *gl(reinterpret_cast<const mu32x4 *>(kb + rc * a.ks[2] + ch * 8));
    const mu32x4 y = *gl(reinterpret_cast<const mu32x4 *>(vb + rc * a.vs[2] + ch * 8));
    rk[j] = ok ? x : mu32x4{0u, 0u, 0u, 0u};
    rv[j] = ok ? y : mu32x4{0u, 0u, 0u, 0u};
  }
#pragma unroll
  for (int j = 0; j < NKV; ++j) {
    const int i = tid + j * kThreads, row = i / CH, ch = i % CH;
    if (row < kKeys) {
      *reinterpret_cast<mu32x4 *>(Ks + row * LD + ch * 8) = rk[j];
      *reinterpret_cast<mu32x4 *>(Vs + row * LD + ch * 8) = rv[j];
      union { mu32x4 u; S s[8]; } x;
      x.u = rk[j];
#pragma unroll
      for (int e = 0; e < 8; ++e) Kt[(ch * 8 + e) * kLdKey + row] = x.s[e];
    }
  }

  mf32x4 accK[TPW][kKeyTiles], accV[TPW][kKeyTiles];
#pragma unroll
  for (int u = 0; u < TPW; ++u)
#pragma unroll
    for (int t = 0; t < kKeyTiles; ++t) accK[u][t] = accV[u][t] = mf32x4{0.f, 0.f, 0.f, 0.f};

  const float sl2 = a.scale * 1.4426950408889634f;  // scores in units of log2 e: p = exp2(s - max)
  const bool dead_d = HALF_D && g >= 2;             // lanes of the trailing half k-step over the head dimension
  const bool dead_k = g >= 2;                       // and over the keys (64 .. 79 of 96)

  for (int blk = blk0; blk < blk1; ++blk) {
    __syncthreads();  // the previous block's readers of Qs / Gs / Pt / dSt are done (first block: K / V / K^T are staged)
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      const int i = tid + j * kThreads, row = i / CH, ch = i % CH;
      if (row < kBlockQ) {
        *reinterpret_cast<mu32x4 *>(Qs + row * LD + ch * 8) = rq[j];
        *reinterpret_cast<mu32x4 *>(Gs + row * LD + ch * 8) = rg[j];
      }
    }
    __syncthreads();
    if (blk + 1 < blk1) fetch(blk + 1);

    // ---- S^T = K Q^T and dP^T = V dO^T of the wave's 16 queries
    const int qrow = 16 * w + c;  // this lane's query row inside the block (as B operand row and as score owner)
    mf32x4 s[kKeyTiles], dp[kKeyTiles];
#pragma unroll
    for (int t = 0; t < kKeyTiles; ++t) s[t] = dp[t] = mf32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KSD; ++ks) {
      const bool dead = ks == KSD - 1 && dead_d;
      const int col = 32 * ks + 8 * g;
      const frag qf = lds_frag<E>(Qs, qrow, LD, col, dead), gf = lds_frag<E>(Gs, qrow, LD, col, dead);
#pragma unroll
      for (int t = 0; t < kKeyTiles; ++t) {
        s[t] = FmMfma<E>::mma(lds_frag<E>(Ks, 16 * t + c, LD, col, dead), qf, s[t]);
        dp[t] = FmMfma<E>::mma(lds_frag<E>(Vs, 16 * t + c, LD, col, dead), gf, dp[t]);
      }
    }

    // ---- softmax over the keys, delta and dS: lane l owns keys 16 t + 4 g + r of query c; its row mates are lanes l ^ 16, l ^ 32
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < kKeyTiles; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float x = (16 * t + 4 * g + r < Sk) ? s[t][r] * sl2 : -INFINITY;
        s[t][r] = x;
        m = fmaxf(m, x);
      }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < kKeyTiles; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = (16 * t + 4 * g + r < Sk) ? exp2f(s[t][r] - m) : 0.f;
        s[t][r] = p;
        sum += p;
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.f / sum;
    float delta = 0.f;
#pragma unroll
    for (int t = 0; t < kKeyTiles; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] *= inv;
        delta += s[t][r] * dp[t][r];
      }
    delta += __shfl_xor(delta, 16, 64);
    delta += __shfl_xor(delta, 32, 64);
#pragma unroll
    for (int t = 0; t < kKeyTiles; ++t) {
      union { mu32x2 u; S e[4]; } pk;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float ds = s[t][r] * (dp[t][r] - delta);
        pk.e[r] = E::from_f(ds);
        if (a.need_kv) {
          Pt[(16 * t + 4 * g + r) * kLdQry + qrow] = E::from_f(s[t][r]);
          dSt[(16 * t + 4 * g + r) * kLdQry + qrow] = pk.e[r];
        }
      }
      *reinterpret_cast<mu32x2 *>(dSq + qrow * kLdKey + 16 * t + 4 * g) = pk.u;
    }
    __syncthreads();

    // ---- dQ^T = K^T dS^T: lane l holds query c, head-dim columns 16 dt + 4 g + r
    {
      frag dsf[KSK];
#pragma unroll
      for (int ks = 0; ks < KSK; ++ks) dsf[ks] = lds_frag<E>(dSq, qrow, kLdKey, 32 * ks + 8 * g, ks == KSK - 1 && dead_k);
      const int qi = blk * kBlockQ + qrow;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        mf32x4 acc = mf32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KSK; ++ks)
          acc = FmMfma<E>::mma(lds_frag<E>(Kt, 16 * dt + c, kLdKey, 32 * ks + 8 * g, ks == KSK - 1 && dead_k), dsf[ks], acc);
        if (qi < Sq) {
          union { mu32x2 u; S e[4]; } pk;
#pragma unroll
          for (int r = 0; r < 4; ++r) pk.e[r] = E::from_f(acc[r] * a.scale);
          *gl(reinterpret_cast<mu32x2 *>(dqb + (int64_t)qi * a.dqs[2] + 16 * dt + 4 * g)) = pk.u;
        }
      }
    }

    // ---- dK += dS^T Q, dV += P^T dO over the block's 64 queries: lane l holds key 16 t + 4 g + r, head-dim column 16 dt + c
    if (a.need_kv) {
#pragma unroll
      for (int u = 0; u < TPW; ++u) {
        const int dt = w + 4 * u;
        if (dt < NDT) {
#pragma unroll
          for (int ks = 0; ks < kBlockQ / 32; ++ks) {
            const frag bq = lds_frag_col<E>(Qs, 32 * ks + 8 * g, LD, 16 * dt + c);
            const frag bg = lds_frag_col<E>(Gs, 32 * ks + 8 * g, LD, 16 * dt + c);
#pragma unroll
            for (int t = 0; t < kKeyTiles; ++t) {
              accK[u][t] = FmMfma<E>::mma(lds_frag<E>(dSt, 16 * t + c, kLdQry, 32 * ks + 8 * g, false), bq, accK[u][t]);
              accV[u][t] = FmMfma<E>::mma(lds_frag<E>(Pt, 16 * t + c, kLdQry, 32 * ks + 8 * g, false), bg, accV[u][t]);
            }
          }
        }
      }
    }
  }

  // ---- this workgroup's slab: [dK | dV][80][D] f32 (rows >= Sk are zeros; the fold does not read them)
  if (a.need_kv) {
    float *slab_k = a.ws + (int64_t)blockIdx.x * (2 * kKeys * D), *slab_v = slab_k + kKeys * D;
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
      const int dt = w + 4 * u;
      if (dt < NDT) {
#pragma unroll
        for (int t = 0; t < kKeyTiles; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int o = (16 * t + 4 * g + r) * D + 16 * dt + c;
            *gl(slab_k + o) = accK[u][t][r] * a.scale;
            *gl(slab_v + o) = accV[u][t][r];
          }
      }
    }
  }
}

// dK / dV [B, H, Sk, D] = the sum of a (batch, head)'s slabs in slab order: one thread per 4 consecutive columns
template <class E, int D>
__global__ __launch_bounds__(kThreads) void attn_short_fold_kernel(const AttnShortFoldArgs<typename E::storage> a, int64_t total) {
  using S = typename E::storage;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  constexpr int C4 = D / 4;
  const int c4 = (int)(i % C4);
  int64_t r = i / C4;
  const int key = (int)(r % a.Sk);
  r /= a.Sk;
  const int mat = (int)(r & 1);
  const int64_t bh = r >> 1;
  const float *p = a.ws + (bh * a.slabs * 2 + mat) * (int64_t)(kKeys * D) + key * D + c4 * 4;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  for (int sl = 0; sl < a.slabs; ++sl, p += 2 * kKeys * D) {
    const float4 x = gl_ld4(p);
    s0 += x.x; s1 += x.y; s2 += x.z; s3 += x.w;
  }
  union { mu32x2 u; S e[4]; } pk;
  pk.e[0] = E::from_f(s0); pk.e[1] = E::from_f(s1); pk.e[2] = E::from_f(s2); pk.e[3] = E::from_f(s3);
  const int b = (int)(bh / a.H), h = (int)(bh % a.H);
  S *dst = mat == 0 ? a.dk + b * a.dks[0] + h * a.dks[1] + key * a.dks[2] : a.dv + b * a.dvs[0] + h * a.dvs[1] + key * a.dvs[2];
  *gl(reinterpret_cast<mu32x2 *>(dst + c4 * 4)) = pk.u;
}

bool head_dim_ok(int D) { return D == 64 || D == 80 || D == 96 || D == 128 || D == 160; }

}  // namespace
}  // namespace lora_amd

using namespace lora_amd;

extern "C" int lora_amd_attn_short_bwd_supported(int64_t Sq, int32_t Sk, int32_t D, int32_t dtype,
                                                 const int64_t *strides_host, int32_t n_strides) {
  if (Sq < 1 || Sq > (int64_t)1 << 30 || Sk < 1 || Sk > kKeys || !head_dim_ok(D) || dtype != LORA_AMD_BF16) return 0;
  for (int i = 0; i < n_strides; ++i)
    if (strides_host == nullptr || strides_host[i] < 0 || strides_host[i] % 8 != 0) return 0;  // 16-byte rows
  return 1;
}

extern "C" int lora_amd_attn_short_bwd_plan(int32_t B, int32_t H, int64_t Sq, int32_t Sk, int32_t D,
                                            lora_amd_attn_short_plan *plan_host) {
  LORA_AMD_CHECK(plan_host != nullptr, LORA_AMD_EINVAL, "attn_short_bwd_plan: null plan");
  LORA_AMD_CHECK(B >= 1 && H >= 1 && (int64_t)B * H <= 1 << 20, LORA_AMD_EINVAL, "attn_short_bwd_plan: B = %d, H = %d", B, H);
  LORA_AMD_CHECK(lora_amd_attn_short_bwd_supported(Sq, Sk, D, LORA_AMD_BF16, nullptr, 0), LORA_AMD_EUNSUPPORTED,
                 "attn_short_bwd_plan: Sq = %lld, Sk = %d, D = %d unsupported", (long long)Sq, Sk, D);
  // run length: about one workgroup per CU, and at least 4 blocks behind one staging of K / V and one slab
  const int64_t nblk = (Sq + kBlockQ - 1) / kBlockQ, total = nblk * B * H;
  int64_t run = (total + kTargetGroups - 1) / kTargetGroups;
  if (run < kMinRun) run = kMinRun;
  if (run > nblk) run = nblk;
  plan_host->run_blocks = (int32_t)run;
  plan_host->slabs = (int32_t)((nblk + run - 1) / run);
  plan_host->slab_bytes = (int64_t)2 * kKeys * D * sizeof(float);
  plan_host->workspace_bytes = plan_host->slab_bytes * plan_host->slabs * B * H;
  return LORA_AMD_OK;
}

extern "C" int lora_amd_attn_short_bwd(const void *q, const int64_t *q_strides_host, const void *k,
                                       const int64_t *k_strides_host, const void *v, const int64_t *v_strides_host,
                                       const void *dout, const int64_t *dout_strides_host, void *dq,
                                       const int64_t *dq_strides_host, void *dk, const int64_t *dk_strides_host, void *dv,
                                       const int64_t *dv_strides_host, int32_t B, int32_t H, int64_t Sq, int32_t Sk, int32_t D,
                                       float scale, int32_t dtype, void *workspace, size_t workspace_bytes, void *stream) {
  const bool need_kv = dk != nullptr || dv != nullptr;
  LORA_AMD_CHECK(q && k && v && dout && dq && q_strides_host && k_strides_host && v_strides_host && dout_strides_host &&
                     dq_strides_host, LORA_AMD_EINVAL, "attn_short_bwd: null operand");
  LORA_AMD_CHECK(!need_kv || (dk && dv && dk_strides_host && dv_strides_host), LORA_AMD_EINVAL,
                 "attn_short_bwd: dk and dv come together (both or neither)");
  int64_t st[21];
  const int64_t *src[7] = {q_strides_host, k_strides_host, v_strides_host, dout_strides_host, dq_strides_host,
                           need_kv ? dk_strides_host : dq_strides_host, need_kv ? dv_strides_host : dq_strides_host};
  for (int i = 0; i < 7; ++i)
    for (int j = 0; j < 3; ++j) st[3 * i + j] = src[i][j];
  LORA_AMD_CHECK(lora_amd_attn_short_bwd_supported(Sq, Sk, D, dtype, st, 21), LORA_AMD_EUNSUPPORTED,
                 "attn_short_bwd: Sq = %lld, Sk = %d, D = %d, dtype %d or a stride that is no multiple of 8 elements",
                 (long long)Sq, Sk, D, dtype);
  const void *ptrs[7] = {q, k, v, dout, dq, dk, dv};
  for (int i = 0; i < 7; ++i)
    LORA_AMD_CHECK(((uintptr_t)ptrs[i] & 15) == 0, LORA_AMD_EINVAL, "attn_short_bwd: operand %d is not 16-byte aligned", i);
  lora_amd_attn_short_plan plan;
  const int rc = lora_amd_attn_short_bwd_plan(B, H, Sq, Sk, D, &plan);
  if (rc != LORA_AMD_OK) return rc;
  if (need_kv) {
    LORA_AMD_CHECK(workspace != nullptr && ((uintptr_t)workspace & 15) == 0, LORA_AMD_EINVAL,
                   "attn_short_bwd: workspace null or not 16-byte aligned");
    LORA_AMD_CHECK(workspace_bytes >= (size_t)plan.workspace_bytes, LORA_AMD_EWORKSPACE,
                   "attn_short_bwd: workspace %zu < %lld bytes", workspace_bytes, (long long)plan.workspace_bytes);
  }
  using S = bf16_t::storage;
  AttnShortArgs<S> a;
  a.q = (const S *)q; a.k = (const S *)k; a.v = (const S *)v; a.go = (const S *)dout;
  a.dq = (S *)dq;
  a.ws = (float *)workspace;
  for (int j = 0; j < 3; ++j) {
    a.qs[j] = st[j]; a.ks[j] = st[3 + j]; a.vs[j] = st[6 + j]; a.gs[j] = st[9 + j]; a.dqs[j] = st[12 + j];
  }
  a.Sq = (int)Sq; a.Sk = Sk; a.H = H; a.run = plan.run_blocks; a.slabs = plan.slabs; a.need_kv = need_kv ? 1 : 0;
  a.scale = scale;
  AttnShortFoldArgs<S> f;
  f.ws = (const float *)workspace; f.dk = (S *)dk; f.dv = (S *)dv;
  for (int j = 0; j < 3; ++j) { f.dks[j] = st[15 + j]; f.dvs[j] = st[18 + j]; }
  f.Sk = Sk; f.H = H; f.slabs = plan.slabs;
  const unsigned grid = (unsigned)((int64_t)B * H * plan.slabs);
  const int64_t fold_total = (int64_t)B * H * 2 * Sk * (D / 4);
  const unsigned fold_grid = (unsigned)((fold_total + kThreads - 1) / kThreads);
  hipStream_t hs = (hipStream_t)stream;
  by_int<64, 80, 96, 128, 160>(D, [&](auto d) {
    constexpr int DD = decltype(d)::value;
    hipLaunchKernelGGL((attn_short_bwd_kernel<bf16_t, DD>), dim3(grid), dim3(kThreads), 0, hs, a);
    if (need_kv)
      hipLaunchKernelGGL((attn_short_fold_kernel<bf16_t, DD>), dim3(fold_grid), dim3(kThreads), 0, hs, f, fold_total);
    return 0;
  });
  return check_launch("attn_short_bwd");
}
