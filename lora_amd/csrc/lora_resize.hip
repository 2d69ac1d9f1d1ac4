// Resize a LoRA to a lower rank from its factors alone (cli_svd.resize_pairs).
//
// Per site, A = up diag(scale) [N, R], D = down [R, K], dW = A D (never formed):
//   Gu = A^T A,  Gd = D D^T                            resize_gram_kernel   (f64 partials per 256-row block)
//   Gu = E L E^T,  M = L^1/2 E^T Gd E L^1/2 = F S^2 F^T resize_core_kernel   (one workgroup per site, f64 Jacobi in LDS)
//   Pu = (E L^-1/2 F S)[:, :r],  Pd = (S^-1 F^T L^1/2 E^T)[:r]
//   up' = A Pu,  down' = Pd D                          resize_apply_kernel  (f64 accumulation, f32 outputs)
//   largest-|.| entry of every down' row positive      resize_sign_kernel
// Every launch reads one device table with an entry per site (grid.y = site); no workgroup waits for another and there
// are no atomics: partials are summed in block order, so two runs give the same bits.
#include "common.hpp"

namespace lora_amd {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxR = LORA_AMD_MAX_RANK;   // 64
constexpr int kPitch = kMaxR + 1;          // odd pitch: a column walk touches every bank
constexpr int kGramRows = 256;             // rows of A (or D^T) per Gram partial
constexpr int kTile = 64;                  // rows staged in LDS at a time
constexpr int kMaxSweeps = 24;             // Jacobi sweeps before a site gives up (f64, n <= 64: 6-10 expected)

constexpr int kStatusGu = 1, kStatusM = 2, kStatusNonFinite = 4;

__host__ __device__ inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
__host__ __device__ inline int gram_blocks(int64_t rows) { return cdiv(rows, kGramRows); }
__host__ __device__ inline int apply_blocks(int64_t rows) { return cdiv(rows, kTile); }
// doubles of one site's workspace: the Gram partials of both sides, then Pu [R][r] and Pd [r][R]
__host__ __device__ inline int64_t site_doubles(int64_t N, int64_t K, int R, int r) {
  return (int64_t)(gram_blocks(N) + gram_blocks(K)) * R * R + 2 * (int64_t)R * r;
}

// rows [base, base + kTile) of A (row stride R) or of D^T (element (k, j) = down[j K + k]) into X; rows past `rows`: zero
__device__ inline void stage_rows(float (*X)[kPitch], const float *src, bool side_d, int64_t base, int64_t rows, int R,
                                  int64_t K) {
  const int nt = (int)(rows - base < kTile ? rows - base : kTile);
  for (int idx = threadIdx.x; idx < kTile * R; idx += kThreads) {
    int t, j;
    if (side_d) { j = idx / kTile; t = idx % kTile; } else { t = idx / R; j = idx % R; }
    float v = 0.f;
    if (t < nt) v = side_d ? gl(src)[(int64_t)j * K + base + t] : gl(src)[(base + t) * R + j];
    X[t][j] = v;
  }
}

__global__ __launch_bounds__(kThreads) void resize_gram_kernel(const lora_amd_resize_site *__restrict__ sites,
                                                               unsigned char *__restrict__ ws) {
  const lora_amd_resize_site s = sites[blockIdx.y];
  const int R = s.R, bn = gram_blocks(s.N), bk = gram_blocks(s.K), b = blockIdx.x;
  if (b >= bn + bk) return;
  const bool side_d = b >= bn;
  const int64_t rows = side_d ? s.K : s.N;
  const int64_t row0 = (int64_t)(side_d ? b - bn : b) * kGramRows;
  const float *src = side_d ? s.down : s.up;
  __shared__ float X[kTile][kPitch];
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  for (int idx = tid; idx < kTile * kPitch; idx += kThreads) (&X[0][0])[idx] = 0.f;   // columns >= R stay zero
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = 0.0;
  for (int t0 = 0; t0 < kGramRows; t0 += kTile) {
    const int64_t base = row0 + t0;
    if (base >= rows) break;
    __syncthreads();
    stage_rows(X, src, side_d, base, rows, R, s.K);
    __syncthreads();
    const int nt = (int)(rows - base < kTile ? rows - base : kTile);
    for (int t = 0; t < nt; ++t) {
      double xi[4], xj[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) { xi[a] = (double)X[t][ti + 16 * a]; xj[a] = (double)X[t][tj + 16 * a]; }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = fma(xi[a], xj[c], acc[a][c]);   // f32 x f32 is exact in f64
    }
  }
  double *part = reinterpret_cast<double *>(ws + s.ws_offset) + (int64_t)b * R * R;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = ti + 16 * a, j = tj + 16 * c;
      if (i < R && j < R) gl(part)[i * R + j] = acc[a][c];
    }
}

// pair k of step `step` of the round-robin ordering of n = m + 1 players (m odd): every index meets every other once a sweep
__device__ inline void rr_pair(int k, int step, int m, int &p, int &q) {
  int a, b;
  if (k == 0) { a = m; b = step; } else { a = (step + k) % m; b = (step - k + m) % m; }
  p = a < b ? a : b;
  q = a < b ? b : a;
}

// rotation parameters and index pairs of one Jacobi step, and the sweeps' "a rotation happened" flags
struct JacobiStep {
  double c[kMaxR / 2], s[kMaxR / 2], t[kMaxR / 2];
  int p[kMaxR / 2], q[kMaxR / 2];
  int flag[2];
};

// Cyclic two-sided Jacobi on the symmetric n x n matrix A (n even), eigenvectors in the columns of V (set to I here).
// One step rotates the n / 2 disjoint pairs of the ordering at once: the angles from the current A, then every 2 x 2 block
// (pair k1, pair k2), k1 <= k2, is rotated from both sides by one thread and mirrored, so A stays exactly symmetric.
// Off-diagonal entries at or below `thr` are left alone; a sweep without a rotation ends the iteration.
// Returns the sweeps run, or -1 after kMaxSweeps.  Workgroup barriers only: two per step.  Which blocks and which (row, pair)
// items a thread owns is fixed for the whole solve (no division inside the step loop); the step's pairs come from LDS.
__device__ int jacobi_sym(double (*A)[kPitch], double (*V)[kPitch], int n, double thr, JacobiStep &js) {
  constexpr int kAItems = (kMaxR / 2) * (kMaxR / 2) / kThreads, kVItems = kMaxR * (kMaxR / 2) / kThreads;
  const int tid = threadIdx.x, h = n >> 1, m = n - 1;
  for (int idx = tid; idx < n * n; idx += kThreads) V[idx / n][idx % n] = (idx / n == idx % n) ? 1.0 : 0.0;
  int ak1[kAItems], ak2[kAItems], vi[kVItems], vk[kVItems];
#pragma unroll
  for (int u = 0; u < kAItems; ++u) {
    const int it = tid + u * kThreads;
    ak1[u] = it / h;
    ak2[u] = it % h;
    if (it >= h * h || ak1[u] > ak2[u]) ak1[u] = -1;
  }
#pragma unroll
  for (int u = 0; u < kVItems; ++u) {
    const int it = tid + u * kThreads;
    vi[u] = it < n * h ? it / h : -1;
    vk[u] = it % h;
  }
  for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
    if (tid == 0) js.flag[sweep & 1] = 0;
    __syncthreads();
    for (int step = 0; step < m; ++step) {
      if (tid < h) {
        int p, q;
        rr_pair(tid, step, m, p, q);
        const double apq = A[p][q];
        double c = 1.0, sn = 0.0, t = 0.0;
        if (fabs(apq) > thr) {
          const double tau = (A[q][q] - A[p][p]) / (2.0 * apq);
          t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
          c = 1.0 / sqrt(1.0 + t * t);
          sn = t * c;
          js.flag[sweep & 1] = 1;
        }
        js.c[tid] = c; js.s[tid] = sn; js.t[tid] = t;
        js.p[tid] = p; js.q[tid] = q;
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < kAItems; ++u) {
        const int k1 = ak1[u], k2 = ak2[u];
        if (k1 < 0) continue;
        const int p1 = js.p[k1], q1 = js.q[k1];
        if (k1 == k2) {
          const double apq = A[p1][q1], t = js.t[k1];
          A[p1][p1] -= t * apq;
          A[q1][q1] += t * apq;
          if (t != 0.0) { A[p1][q1] = 0.0; A[q1][p1] = 0.0; }
          continue;
        }
        const int p2 = js.p[k2], q2 = js.q[k2];
        const double c1 = js.c[k1], s1 = js.s[k1], c2 = js.c[k2], s2 = js.s[k2];
        const double b00 = A[p1][p2], b01 = A[p1][q2], b10 = A[q1][p2], b11 = A[q1][q2];
        const double t00 = c2 * b00 - s2 * b01, t01 = s2 * b00 + c2 * b01;
        const double t10 = c2 * b10 - s2 * b11, t11 = s2 * b10 + c2 * b11;
        const double n00 = c1 * t00 - s1 * t10, n01 = c1 * t01 - s1 * t11;
        const double n10 = s1 * t00 + c1 * t10, n11 = s1 * t01 + c1 * t11;
        A[p1][p2] = n00; A[p2][p1] = n00;
        A[p1][q2] = n01; A[q2][p1] = n01;
        A[q1][p2] = n10; A[p2][q1] = n10;
        A[q1][q2] = n11; A[q2][q1] = n11;
      }
#pragma unroll
      for (int u = 0; u < kVItems; ++u) {
        const int i = vi[u], k = vk[u];
        if (i < 0) continue;
        const int p = js.p[k], q = js.q[k];
        const double c = js.c[k], sn = js.s[k], vp = V[i][p], vq = V[i][q];
        V[i][p] = c * vp - sn * vq;
        V[i][q] = sn * vp + c * vq;
      }
      __syncthreads();
    }
    if (js.flag[sweep & 1] == 0) return sweep + 1;
  }
  return -1;
}

// A[i][j] (n x n, zero outside R x R) = sum of `nblocks` R x R partials in block order, times sc[i] sc[j] when sc != null
__device__ inline void sum_partials(double (*A)[kPitch], const double *part, int nblocks, int R, int n, const float *sc) {
  for (int idx = threadIdx.x; idx < n * n; idx += kThreads) {
    const int i = idx / n, j = idx % n;
    double v = 0.0;
    if (i < R && j < R) {
      for (int b = 0; b < nblocks; ++b) v += gl(part)[(int64_t)b * R * R + i * R + j];
      if (sc != nullptr) v *= (double)gl(sc)[i] * (double)gl(sc)[j];
    }
    A[i][j] = v;
  }
}

__global__ __launch_bounds__(kThreads) void resize_core_kernel(const lora_amd_resize_site *__restrict__ sites,
                                                               unsigned char *__restrict__ ws, double tol,
                                                               double *__restrict__ s_out, int32_t *__restrict__ status) {
  const lora_amd_resize_site s = sites[blockIdx.x];
  const int R = s.R, r = s.r, tid = threadIdx.x;
  const int n = (R + 1) & ~1;
  const int bn = gram_blocks(s.N), bk = gram_blocks(s.K);
  __shared__ double A[kMaxR][kPitch], V[kMaxR][kPitch], W[kMaxR][kPitch];
  __shared__ double lam[kMaxR], sq[kMaxR], isq[kMaxR], sg[kMaxR];
  __shared__ JacobiStep js;
  __shared__ int ord[kMaxR];
  double *part = reinterpret_cast<double *>(ws + s.ws_offset);
  double *Pu = part + (int64_t)(bn + bk) * R * R, *Pd = Pu + (int64_t)R * r;
  int st = 0;

  // ---- Gu = E diag(lam) E^T
  sum_partials(A, part, bn, R, n, s.scale);
  __syncthreads();
  double trace = 0.0;
  for (int i = 0; i < R; ++i) trace += A[i][i];
  if (!(fabs(trace) <= 1.7e308)) st |= kStatusNonFinite;
  __syncthreads();
  if (jacobi_sym(A, V, n, 1e-17 * fabs(trace), js) < 0) st |= kStatusGu;
  if (tid < R) lam[tid] = A[tid][tid];
  __syncthreads();
  double lmax = 0.0;
  for (int i = 0; i < R; ++i) lmax = lam[i] > lmax ? lam[i] : lmax;
  if (tid < R) {   // eigenvalues at or below tol * lam_max count as zero (pseudo-inverse)
    const double l = lam[tid], root = (l > tol * lmax && l > 0.0) ? sqrt(l) : 0.0;
    sq[tid] = root;
    isq[tid] = root > 0.0 ? 1.0 / root : 0.0;
  }
  // ---- M = L^1/2 E^T Gd E L^1/2
  sum_partials(A, part + (int64_t)bn * R * R, bk, R, n, nullptr);
  __syncthreads();
  for (int idx = tid; idx < R * R; idx += kThreads) {   // W = Gd E L^1/2
    const int i = idx / R, j = idx % R;
    double v = 0.0;
    for (int k = 0; k < R; ++k) v = fma(A[i][k], V[k][j], v);
    W[i][j] = v * sq[j];
  }
  __syncthreads();
  for (int idx = tid; idx < R * R; idx += kThreads) {   // upper triangle, mirrored
    const int i = idx / R, j = idx % R;
    if (i > j) continue;
    double v = 0.0;
    for (int k = 0; k < R; ++k) v = fma(V[k][i], W[k][j], v);
    v *= sq[i];
    A[i][j] = v;
    A[j][i] = v;
  }
  __syncthreads();
  for (int idx = tid; idx < R * R; idx += kThreads) W[idx / R][idx % R] = V[idx / R][idx % R];   // E
  __syncthreads();
  trace = 0.0;
  for (int i = 0; i < R; ++i) trace += A[i][i];
  if (!(fabs(trace) <= 1.7e308)) st |= kStatusNonFinite;
  __syncthreads();
  if (jacobi_sym(A, V, n, 1e-17 * fabs(trace), js) < 0) st |= kStatusM;
  if (tid < R) lam[tid] = A[tid][tid];
  __syncthreads();
  double smax = 0.0;
  for (int i = 0; i < R; ++i) smax = lam[i] > smax ? lam[i] : smax;
  if (tid < R) {
    const double l = lam[tid];
    sg[tid] = (l > tol * smax && l > 0.0) ? sqrt(l) : 0.0;
    int pos = 0;   // descending order; equal values keep their index order
    for (int i = 0; i < R; ++i) pos += (lam[i] > l || (lam[i] == l && i < tid)) ? 1 : 0;
    ord[pos] = tid;
  }
  __syncthreads();
  if (tid < R) gl(s_out)[(int64_t)blockIdx.x * kMaxR + tid] = sg[ord[tid]];
  // ---- Pu = (E L^-1/2 F S)[:, :r],  Pd = (S^-1 F^T L^1/2 E^T)[:r]      (E in W, F in V)
  for (int idx = tid; idx < R * r; idx += kThreads) {
    const int i = idx / r, jj = idx % r, o = ord[jj];
    const double sv = sg[o];
    double u = 0.0, d = 0.0;
    if (sv > 0.0) {
      for (int k = 0; k < R; ++k) {
        const double e = W[i][k], f = V[k][o];
        u = fma(e * isq[k], f, u);
        d = fma(e * sq[k], f, d);
      }
      u *= sv;
      d /= sv;
    }
    gl(Pu)[i * r + jj] = u;
    gl(Pd)[jj * R + i] = d;
  }
  if (tid == 0) gl(status)[blockIdx.x] = st;
}

__global__ __launch_bounds__(kThreads) void resize_apply_kernel(const lora_amd_resize_site *__restrict__ sites,
                                                                const unsigned char *__restrict__ ws) {
  const lora_amd_resize_site s = sites[blockIdx.y];
  const int R = s.R, r = s.r, an = apply_blocks(s.N), ak = apply_blocks(s.K), b = blockIdx.x;
  if (b >= an + ak) return;
  const bool side_d = b >= an;
  const int64_t rows = side_d ? s.K : s.N;
  const int64_t base = (int64_t)(side_d ? b - an : b) * kTile;
  __shared__ float X[kTile][kPitch];
  __shared__ double P[kMaxR][kMaxR];
  const double *part = reinterpret_cast<const double *>(ws + s.ws_offset);
  const double *Pu = part + (int64_t)(gram_blocks(s.N) + gram_blocks(s.K)) * R * R, *Pd = Pu + (int64_t)R * r;
  const int tid = threadIdx.x;
  for (int idx = tid; idx < R * r; idx += kThreads) {   // P[i][j]: the input's column i into output j
    const int i = idx / r, j = idx % r;
    P[i][j] = side_d ? gl(Pd)[j * R + i] : gl(Pu)[i * r + j] * (s.scale != nullptr ? (double)gl(s.scale)[i] : 1.0);
  }
  stage_rows(X, side_d ? s.down : s.up, side_d, base, rows, R, s.K);
  __syncthreads();
  const int t = tid & 63;
  if (base + t >= rows) return;
  for (int j = tid >> 6; j < r; j += kThreads / 64) {
    double acc = 0.0;
    for (int i = 0; i < R; ++i) acc = fma((double)X[t][i], P[i][j], acc);
    if (side_d) gl(s.down_out)[(int64_t)j * s.K + base + t] = (float)acc;
    else gl(s.up_out)[(base + t) * r + j] = (float)acc;
  }
}

// cli_svd._fix_signs: the largest-|.| entry of down' row j (the first one among equals) becomes positive; up' column j follows
__global__ __launch_bounds__(kThreads) void resize_sign_kernel(const lora_amd_resize_site *__restrict__ sites) {
  const lora_amd_resize_site s = sites[blockIdx.y];
  const int j = blockIdx.x, tid = threadIdx.x;
  if (j >= s.r) return;
  float *row = s.down_out + (int64_t)j * s.K;
  __shared__ float babs[kThreads];
  __shared__ int64_t bidx[kThreads];
  float best = -1.f;
  int64_t at = 0;
  for (int64_t k = tid; k < s.K; k += kThreads) {
    const float a = fabsf(gl(row)[k]);
    if (a > best) { best = a; at = k; }
  }
  babs[tid] = best;
  bidx[tid] = at;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (tid < w) {
      const float oa = babs[tid + w];
      const int64_t oi = bidx[tid + w];
      if (oa > babs[tid] || (oa == babs[tid] && oi < bidx[tid])) { babs[tid] = oa; bidx[tid] = oi; }
    }
    __syncthreads();
  }
  __shared__ int negative;
  if (tid == 0) negative = gl(row)[bidx[0]] < 0.f ? 1 : 0;
  __syncthreads();
  if (!negative) return;
  for (int64_t k = tid; k < s.K; k += kThreads) gl(row)[k] = -gl(row)[k];
  for (int64_t i = tid; i < s.N; i += kThreads) gl(s.up_out)[i * s.r + j] = -gl(s.up_out)[i * s.r + j];
}

// 0: the kernels take the site; else the reason as an error code (message set)
int site_native(int64_t N, int64_t K, int32_t R, int32_t r, const char *what) {
  LORA_AMD_CHECK(R >= 1 && R <= kMaxR, LORA_AMD_ERANK, "%s: rank %d outside [1, %d]", what, R, kMaxR);
  LORA_AMD_CHECK(r >= 1 && r <= R, LORA_AMD_ERANK, "%s: target rank %d outside [1, %d]", what, r, R);
  LORA_AMD_CHECK(N >= 1 && K >= 1 && N < (1ll << 31) && K < (1ll << 31), LORA_AMD_EINVAL, "%s: bad shape %lld x %lld", what,
                 (long long)N, (long long)K);
  return LORA_AMD_OK;
}

int check_table(const char *what, const lora_amd_resize_site *sites_dev, int32_t n, const lora_amd_resize_table_t *geo) {
  LORA_AMD_CHECK(sites_dev != nullptr && geo != nullptr && n >= 1, LORA_AMD_EINVAL, "%s: null table or no sites", what);
  LORA_AMD_CHECK((uintptr_t)sites_dev % 16 == 0, LORA_AMD_EINVAL, "%s: the site table is not 16-byte aligned", what);
  LORA_AMD_CHECK(geo->n_sites == n && geo->gram_grid >= 1 && geo->apply_grid >= 1 && geo->sign_grid >= 1 &&
                     geo->sign_grid <= kMaxR && geo->workspace_bytes > 0,
                 LORA_AMD_EINVAL, "%s: the geometry was not planned for this table (lora_amd_resize_table_plan)", what);
  return LORA_AMD_OK;
}

int check_ws(const char *what, const lora_amd_resize_table_t *geo, const void *ws, size_t ws_bytes) {
  LORA_AMD_CHECK(ws != nullptr && (uintptr_t)ws % 16 == 0, LORA_AMD_EINVAL, "%s: null or misaligned workspace", what);
  LORA_AMD_CHECK((int64_t)ws_bytes >= geo->workspace_bytes, LORA_AMD_EWORKSPACE, "%s: workspace of %zu bytes, %lld needed", what,
                 ws_bytes, (long long)geo->workspace_bytes);
  return LORA_AMD_OK;
}

}  // namespace
}  // namespace lora_amd

using namespace lora_amd;

extern "C" int lora_amd_resize_plan(int64_t N, int64_t K, int32_t R, int32_t r, int32_t dtype, const void *up,
                                    const void *down, lora_amd_resize_plan_t *out) {
  LORA_AMD_CHECK(out != nullptr, LORA_AMD_EINVAL, "resize_plan: null plan");
  *out = lora_amd_resize_plan_t{};
  if (int rc = site_native(N, K, R, r, "resize_plan")) return rc == LORA_AMD_ERANK ? rc : LORA_AMD_OK;   // native = 0
  if (dtype != LORA_AMD_F32 || ((uintptr_t)up | (uintptr_t)down) % 16 != 0) return LORA_AMD_OK;
  out->native = 1;
  out->gram_blocks_n = gram_blocks(N);
  out->gram_blocks_k = gram_blocks(K);
  out->apply_blocks_n = apply_blocks(N);
  out->apply_blocks_k = apply_blocks(K);
  out->workspace_bytes = (site_doubles(N, K, R, r) * 8 + 255) / 256 * 256;
  return LORA_AMD_OK;
}

extern "C" int lora_amd_resize_table_plan(lora_amd_resize_site *sites_host, int32_t n_sites, lora_amd_resize_table_t *out) {
  LORA_AMD_CHECK(sites_host != nullptr && out != nullptr && n_sites >= 1, LORA_AMD_EINVAL, "resize_table_plan: null table or no sites");
  lora_amd_resize_table_t g{};
  g.n_sites = n_sites;
  for (int32_t i = 0; i < n_sites; ++i) {
    lora_amd_resize_site &s = sites_host[i];
    if (int rc = site_native(s.N, s.K, s.R, s.r, "resize_table_plan")) return rc;
    LORA_AMD_CHECK(s.up && s.down && s.up_out && s.down_out, LORA_AMD_EINVAL, "resize_table_plan: site %d: null pointer", i);
    LORA_AMD_CHECK(((uintptr_t)s.up | (uintptr_t)s.down) % 16 == 0 && ((uintptr_t)s.up_out | (uintptr_t)s.down_out | (uintptr_t)s.scale) % 4 == 0,
                   LORA_AMD_EINVAL, "resize_table_plan: site %d: factors must be 16-byte aligned", i);
    s.ws_offset = g.workspace_bytes;
    g.workspace_bytes += (site_doubles(s.N, s.K, s.R, s.r) * 8 + 255) / 256 * 256;
    const int gg = gram_blocks(s.N) + gram_blocks(s.K), ag = apply_blocks(s.N) + apply_blocks(s.K);
    g.gram_grid = gg > g.gram_grid ? gg : g.gram_grid;
    g.apply_grid = ag > g.apply_grid ? ag : g.apply_grid;
    g.sign_grid = s.r > g.sign_grid ? s.r : g.sign_grid;
  }
  LORA_AMD_CHECK(n_sites <= 65535, LORA_AMD_EINVAL, "resize_table_plan: at most 65535 sites per table");
  *out = g;
  return LORA_AMD_OK;
}

extern "C" int lora_amd_resize_gram(const lora_amd_resize_site *sites_dev, int32_t n_sites,
                                    const lora_amd_resize_table_t *geo_host, void *workspace, size_t workspace_bytes,
                                    void *stream) {
  if (int rc = check_table("resize_gram", sites_dev, n_sites, geo_host)) return rc;
  if (int rc = check_ws("resize_gram", geo_host, workspace, workspace_bytes)) return rc;
  hipLaunchKernelGGL(resize_gram_kernel, dim3((unsigned)geo_host->gram_grid, (unsigned)n_sites), dim3(kThreads), 0,
                     (hipStream_t)stream, sites_dev, (unsigned char *)workspace);
  return check_launch("lora_amd_resize_gram");
}

extern "C" int lora_amd_resize_core(const lora_amd_resize_site *sites_dev, int32_t n_sites,
                                    const lora_amd_resize_table_t *geo_host, void *workspace, size_t workspace_bytes,
                                    float tol, double *s_out, int32_t *status, void *stream) {
  if (int rc = check_table("resize_core", sites_dev, n_sites, geo_host)) return rc;
  if (int rc = check_ws("resize_core", geo_host, workspace, workspace_bytes)) return rc;
  LORA_AMD_CHECK(s_out != nullptr && status != nullptr && (uintptr_t)s_out % 8 == 0 && (uintptr_t)status % 4 == 0 && tol >= 0.f &&
                     tol < 1.f,
                 LORA_AMD_EINVAL, "resize_core: null or misaligned S / status, or tol outside [0, 1)");
  hipLaunchKernelGGL(resize_core_kernel, dim3((unsigned)n_sites), dim3(kThreads), 0, (hipStream_t)stream, sites_dev,
                     (unsigned char *)workspace, (double)tol, s_out, status);
  return check_launch("lora_amd_resize_core");
}

extern "C" int lora_amd_resize_apply(const lora_amd_resize_site *sites_dev, int32_t n_sites,
                                     const lora_amd_resize_table_t *geo_host, const void *workspace, size_t workspace_bytes,
                                     void *stream) {
  if (int rc = check_table("resize_apply", sites_dev, n_sites, geo_host)) return rc;
  if (int rc = check_ws("resize_apply", geo_host, workspace, workspace_bytes)) return rc;
  hipLaunchKernelGGL(resize_apply_kernel, dim3((unsigned)geo_host->apply_grid, (unsigned)n_sites), dim3(kThreads), 0,
                     (hipStream_t)stream, sites_dev, (const unsigned char *)workspace);
  return check_launch("lora_amd_resize_apply");
}

extern "C" int lora_amd_resize_sign(const lora_amd_resize_site *sites_dev, int32_t n_sites,
                                    const lora_amd_resize_table_t *geo_host, void *stream) {
  if (int rc = check_table("resize_sign", sites_dev, n_sites, geo_host)) return rc;
  hipLaunchKernelGGL(resize_sign_kernel, dim3((unsigned)geo_host->sign_grid, (unsigned)n_sites), dim3(kThreads), 0,
                     (hipStream_t)stream, sites_dev);
  return check_launch("lora_amd_resize_sign");
}
