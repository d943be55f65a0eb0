// libdvae_sep_hip.so (include/dvae_sep_hip.h): the entropies behind the SEPIN / WSEPIN separability scores of Do & Tran 2020,
// estimated like the ELBO decomposition (elbo_decomp.hip) on S samples z_s ~ q(z|x_n(s)) against the aggregate posterior
// q(z) = 1/N sum_n q(z|x_n) of the whole data set.  With t_d(s, n) = log N(z_sd; mu_nd, exp(logvar_nd)):
//     log q_{!=i}(z_s) = logsumexp_{n<N} sum_{d != i} t_d(s, n) - log N      for EVERY i < D  (leave-one-out joint log-density)
//     log q(z_s)       = logsumexp_{n<N} sum_{d < D}  t_d(s, n) - log N      (the joint one, from the same terms)
// -- the S x N x D pass of k_joint_lse with D + 1 results instead of one: every term is formed once and feeds D + 1 online
// logsumexps -- and the conditional entropy per dimension, which needs only the sample's own row.
//
// Decomposition, as k_joint_lse: thread = one sample s with z_s in registers, workgroup = 256 consecutive samples, gridDim.y =
// chunks of the data set.  Per data point ONE contiguous record {mu[DP], -0.5 exp(-logvar)[DP], c[DP]} with c_d = -0.5 (log 2pi +
// logvar_d) PER DIMENSION (n-major, prepared once): wave-uniform in the main loop, so it arrives through scalar loads.  Each
// thread keeps DP + 1 states (running max, sum), rescaled once per LOO_U data points.  D <= 16 is padded to an even DP: a padding
// dimension has z = 0, mu = 0, iv = 0, c = 0 and contributes exactly 0.  The table is padded to whole chunks with records whose
// every term is -inf (c_d = -inf in ALL DP >= 2 columns, so that every leave-one-out sum still holds one; their iv is 1, not 0:
// an overflowed square times 0 would be NaN), so the main loop has no tail.  D > 16: run-time D, z of the workgroup in LDS, and
// the D + 1 states cut into groups of DVAE_SEP_GROUP across gridDim.z, each group recomputing the terms (the joint log-density
// is "leave out dimension D", a dimension whose term is 0).  Chunk partials are merged in chunk order; every sum has a fixed
// order (no atomics).
//
// THE NUMERICAL RULE.  sum_{d != i} t_d is NEVER formed as T - t_i with T = sum_d t_d: it is the sum of a prefix t_0 + .. +
// t_{i-1} and a suffix t_{i+1} + .. + t_{DP-1}, additions only.  With a factor-aligned code and sharp posteriors a data point
// that differs from the sample's own in dimension i ALONE has t_i ~ T ~ -1e5, and its leave-one-out density is still one of the
// dominant ones: T - t_i would keep an absolute error of ulp(1e5) ~ 1e-2 in an exponent of order 1.  Emulated in fp32 on the
// grid tables of tests/sep_ref.py the subtracting form misses the per-sample tolerance by three to four orders of magnitude and
// the adding form stays well inside it (tests/test_sep_host.py holds both).  The same kind of trap as the
// matrix-product form that the header of elbo_decomp.hip explains: large terms that cancel must never be formed.
#include <float.h>
#include <math.h>
#include "../../include/dvae_sep_hip.h"
#include "common.h"
#include "last_error.h"

namespace dvae {

namespace {

#define LOO_TARGET_WGS 2048            // workgroups that fill the device: 256 CUs x 8 (4 waves each)
#define LOO_U 4                        // data points per rescale of the states: 5 v_exp_f32 per 4 densities of a state

// record of data point n at rec + n * 3 DP: mu[0..DP), hiv = -0.5 exp(-logvar) [0..DP), c[0..DP).  Rows n >= N (padding up to
// whole chunks): c = -inf in every column, hiv = -0.5.  Columns d >= D of a real row: all three 0.
__global__ __launch_bounds__(256) void k_loo_prep(const float* __restrict__ mu, const float* __restrict__ lv, long N, long Npad,
                                                  int D, int DP, float* __restrict__ rec) {
  const long n = blockIdx.x * 256L + threadIdx.x;
  if (n >= Npad) return;
  float* r = rec + n * (3 * DP);
  for (int d = 0; d < DP; ++d) {
    float m = 0.f, h = 0.f, c = 0.f;
    if (n >= N) {
      h = -0.5f;
      c = -INFINITY;
    } else if (d < D) {
      const float l = lv[n * D + d];
      m = mu[n * D + d];
      h = -0.5f * expf(-l);
      c = gauss_c(l);
    }
    r[d] = m;
    r[DP + d] = h;
    r[2 * DP + d] = c;
  }
}

// log_density_gaussian (utils/math.py:48-50) of one dimension from its record entries
__device__ __forceinline__ float loo_term(float z, float mu, float hiv, float c) {
  const float diff = z - mu;
  return fmaf(diff * diff, hiv, c);
}

// v[i] = sum_{d != i} t[d] for i < DP, v[DP] = sum_d t[d]: prefix + suffix, additions only (see the header: never T - t_i)
template <int DP>
__device__ __forceinline__ void loo_sums(const float (&t)[DP], float (&v)[DP + 1]) {
  static_assert(DP >= 2, "a leave-one-out sum needs another term");
  float suf[DP];                                            // suf[d] = t[d+1] + .. + t[DP-1], d <= DP - 2
  suf[DP - 2] = t[DP - 1];
#pragma unroll
  for (int d = DP - 3; d >= 0; --d) suf[d] = t[d + 1] + suf[d + 1];
  float pre = t[0];                                         // t[0] + .. + t[d-1]
  v[0] = suf[0];
#pragma unroll
  for (int d = 1; d < DP - 1; ++d) {
    v[d] = pre + suf[d];
    pre += t[d];
  }
  v[DP - 1] = pre;
  v[DP] = pre + t[DP - 1];
}

// lse_fold8 of latent_math.h for NS states at once and U values per rescale; values may be -inf (see there)
template <int U, int NS>
__device__ __forceinline__ void loo_fold(const float (&v)[U][NS], float (&m)[NS], float (&acc)[NS]) {
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    float mx = m[i];
#pragma unroll
    for (int u = 0; u < U; ++u) mx = fmaxf(mx, v[u][i]);
    const float sh = mx > -INFINITY ? mx : 0.f;
    float t = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) t += __expf(v[u][i] - sh);
    acc[i] = acc[i] * __expf(m[i] - sh) + t;
    m[i] = mx;
  }
}

// partials of chunk c, row i (i < D: dimension i left out; i = D: the joint): part + ((c (D+1) + i) 2) S: [0][s] = running max,
// [1][s] = sum of exp(density - max) over the chunk's data points
__device__ __forceinline__ void loo_store(float* __restrict__ part, int D, long S, long s, int i, float m, float acc) {
  float* p = part + (((long)blockIdx.y * (D + 1) + i) * 2) * S;
  p[s] = m;
  p[S + s] = acc;
}

template <int DP>
__global__ __launch_bounds__(256) void k_loo_lse(const float* __restrict__ z, const float* __restrict__ rec, int D, long S,
                                                 int chunk, float* __restrict__ part) {
  constexpr int R = 3 * DP, NS = DP + 1;
  const long s = blockIdx.x * 256L + threadIdx.x;
  float zr[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) zr[d] = (s < S && d < D) ? z[s * D + d] : 0.f;
  const float* r = rec + (long)blockIdx.y * chunk * R;        // wave-uniform: scalar loads
  float m[NS], acc[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) { m[i] = -INFINITY; acc[i] = 0.f; }
  for (int n = 0; n < chunk; n += LOO_U, r += LOO_U * R) {
    float v[LOO_U][NS];
#pragma unroll
    for (int u = 0; u < LOO_U; ++u) {
      const float* q = r + u * R;
      float t[DP];
#pragma unroll
      for (int d = 0; d < DP; ++d) t[d] = loo_term(zr[d], q[d], q[DP + d], q[2 * DP + d]);
      loo_sums<DP>(t, v[u]);
    }
    loo_fold<LOO_U, NS>(v, m, acc);
  }
  if (s < S) {
#pragma unroll
    for (int i = 0; i < DP; ++i)
      if (i < D) loo_store(part, D, S, s, i, m[i], acc[i]);
    loo_store(part, D, S, s, D, m[DP], acc[DP]);
  }
}

// D > 16: run-time D (record stride 3 D), z of the workgroup's samples in LDS as [D][256] (a thread reads its own column only:
// conflict-free, no barrier).  The workgroup keeps the states of rows i0 .. i0 + G, i0 = blockIdx.z * G: their own terms t[G] in
// registers, the terms before and after the group as two running sums -- every leave-one-out sum is still additions only.  Row D
// (the joint) leaves out a dimension whose term is 0; rows past D are computed and not stored.
__global__ __launch_bounds__(256) void k_loo_lse_wide(const float* __restrict__ z, const float* __restrict__ rec, int D, long S,
                                                      int chunk, float* __restrict__ part) {
  extern __shared__ float zl[];
  constexpr int G = DVAE_SEP_GROUP;
  const int R = 3 * D, i0 = blockIdx.z * G;
  const long s = blockIdx.x * 256L + threadIdx.x;
  const float* zg = z + (s < S ? s : S - 1) * D;              // (threads past S compute a copy of the last sample, unwritten)
  for (int d = 0; d < D; ++d) zl[d * 256 + threadIdx.x] = zg[d];
  const float* zc = zl + threadIdx.x;
  float zr[G];
#pragma unroll
  for (int j = 0; j < G; ++j) zr[j] = i0 + j < D ? zc[(i0 + j) * 256] : 0.f;
  const float* r = rec + (long)blockIdx.y * chunk * R;
  float m[G], acc[G];
#pragma unroll
  for (int j = 0; j < G; ++j) { m[j] = -INFINITY; acc[j] = 0.f; }
  for (int n = 0; n < chunk; n += LOO_U, r += LOO_U * R) {
    float v[LOO_U][G];
#pragma unroll
    for (int u = 0; u < LOO_U; ++u) {
      const float* q = r + u * R;
      float before = 0.f, after = 0.f, t[G];
      for (int d = 0; d < i0; ++d) before += loo_term(zc[d * 256], q[d], q[D + d], q[2 * D + d]);
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const int d = i0 + j < D ? i0 + j : D - 1;            // (a dimension past D reads the last one's record and counts 0: no branch)
        const float term = loo_term(zr[j], q[d], q[D + d], q[2 * D + d]);
        t[j] = i0 + j < D ? term : 0.f;
      }
      for (int d = i0 + G; d < D; ++d) after += loo_term(zc[d * 256], q[d], q[D + d], q[2 * D + d]);
      float suf[G];                                           // suf[j] = t[j+1] + .. + t[G-1] + after
      suf[G - 1] = after;
#pragma unroll
      for (int j = G - 2; j >= 0; --j) suf[j] = t[j + 1] + suf[j + 1];
      float pre = before;                                     // before + t[0] + .. + t[j-1]
#pragma unroll
      for (int j = 0; j < G; ++j) {
        v[u][j] = pre + suf[j];
        pre += t[j];
      }
    }
    loo_fold<LOO_U, G>(v, m, acc);
  }
  if (s < S) {
#pragma unroll
    for (int j = 0; j < G; ++j)
      if (i0 + j <= D) loo_store(part, D, S, s, i0 + j, m[j], acc[j]);
  }
}

// merge the chunk partials of every (row, sample) in chunk order: logq[i][s] = logsumexp_n - log N
__global__ __launch_bounds__(256) void k_loo_finish(const float* __restrict__ part, int chunks, long N, int D, long S,
                                                    float* __restrict__ logq) {
  const long s = blockIdx.x * 256L + threadIdx.x;
  const int i = blockIdx.y;
  if (s >= S) return;
  float m = -INFINITY, acc = 0.f;
  for (int c = 0; c < chunks; ++c) {
    const float* p = part + (((long)c * (D + 1) + i) * 2) * S;
    m = lse_merge(m, acc, p[s], p[S + s]);
  }
  logq[(long)i * S + s] = m + logf(acc) - logf((float)N);     // (m = -inf, acc = 0: -inf)
}

// the sum of 1024 per-thread fp64 sums in a fixed order: a tree over LDS; the result in red[0]
__device__ __forceinline__ void loo_tree_sum(double (&red)[1024], double t) {
  red[threadIdx.x] = t;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
}

// H[i] = -1/S sum_s logq[i][s] in fp64: one workgroup per row, thread t sums s = t, t + 1024, ..
__global__ __launch_bounds__(1024) void k_loo_means(const float* __restrict__ logq, long S, double* __restrict__ H) {
  __shared__ double red[1024];
  const float* src = logq + (long)blockIdx.x * S;
  double t = 0.0;
  for (long s = threadIdx.x; s < S; s += 1024) t += (double)src[s];
  loo_tree_sum(red, t);
  if (threadIdx.x == 0) H[blockIdx.x] = -red[0] / (double)S;
}

// H_cond_d[i] = 1/S sum_s 0.5 (log 2pi + logvar[rows[s], i] + eps[s, i]^2) in fp64: one workgroup per dimension
__global__ __launch_bounds__(1024) void k_sep_cond_terms(const float* __restrict__ eps, const float* __restrict__ lv,
                                                         const int64_t* __restrict__ rows, int D, long S, double* __restrict__ H) {
  __shared__ double red[1024];
  const int i = blockIdx.x;
  const double log2pi = log(2.0 * M_PI);
  double t = 0.0;
  for (long s = threadIdx.x; s < S; s += 1024) {
    const double e = (double)eps[s * D + i];
    t += 0.5 * (log2pi + (double)lv[rows[s] * D + i] + e * e);
  }
  loo_tree_sum(red, t);
  if (threadIdx.x == 0) H[i] = red[0] / (double)S;
}

int loo_padded_dim(int D) { return D <= DVAE_SEP_TEMPLATE_D ? (D + 1) & ~1 : D; }

long loo_chunks_of_data(long N) {
  const long c = (N + DVAE_SEP_CHUNK - 1) / DVAE_SEP_CHUNK;
  return c < 1 ? 1 : (c > DVAE_SEP_MAX_CHUNKS ? DVAE_SEP_MAX_CHUNKS : c);
}

// chunks of at least DVAE_SEP_CHUNK data points, and no more of them than it takes to fill the device next to the sample
// blocks (the partials cost chunks * (D + 1) * S * 2 floats)
int loo_chunks(long N, long S) {
  const long sblocks = (S + 255) / 256;
  const long by_s = LOO_TARGET_WGS / sblocks < 1 ? 1 : LOO_TARGET_WGS / sblocks;
  const long c = loo_chunks_of_data(N);
  return (int)(c < by_s ? c : by_s);
}

// bounds of the two workspace parts that are non-decreasing in N and in S (the chunk count itself falls as S grows), as in
// elbo_decomp.hip: table rows <= N + 8 chunks;  chunks * S <= min(chunks_of_data * S, max(S, 256 * target))
size_t loo_table_rows_bound(long N) { return (size_t)N + 8 * (size_t)loo_chunks_of_data(N); }
size_t loo_partial_pairs_bound(long N, long S) {
  const size_t a = (size_t)loo_chunks_of_data(N) * (size_t)S;
  const size_t b = (size_t)S > (size_t)LOO_TARGET_WGS * 256 ? (size_t)S : (size_t)LOO_TARGET_WGS * 256;
  return a < b ? a : b;
}

bool loo_sizes_ok(long N, int D, long S) {
  return N > 0 && N <= 2000000000L && D >= 1 && D <= DVAE_SEP_MAX_D && S > 0 && S <= (1L << 38);
}

}  // namespace
}  // namespace dvae

using namespace dvae;

extern "C" {

int dvae_sep_version(void) { return DVAE_SEP_VERSION; }
const char* dvae_sep_last_error(void) { return last_error(); }

size_t dvae_sep_loo_logq_ws_floats(long N, int D, long S) {
  if (!loo_sizes_ok(N, D, S)) return 0;
  return loo_table_rows_bound(N) * (size_t)(3 * loo_padded_dim(D)) + 2 * (size_t)(D + 1) * loo_partial_pairs_bound(N, S);
}

int dvae_sep_loo_logq(const float* z, const float* mean, const float* logvar, long N, int D, long S, float* ws, float* logq,
                      double* H, void* stream) {
  DVAE_CHECK_ARG(z && mean && logvar && ws && logq && H);
  DVAE_CHECK_ARG(N > 0 && N <= 2000000000L && S > 0 && S <= (1L << 38));
  DVAE_CHECK_ARG(D >= 1 && D <= DVAE_SEP_MAX_D);
  hipStream_t st = (hipStream_t)stream;
  const int DP = loo_padded_dim(D);
  const int chunks = loo_chunks(N, S);
  const int chunk = (int)(((N + chunks - 1) / chunks + 7) / 8 * 8);
  const long Npad = (long)chunks * chunk;
  float* rec = ws;
  float* part = ws + loo_table_rows_bound(N) * (size_t)(3 * DP);
  if ((size_t)Npad > loo_table_rows_bound(N) || (size_t)chunks * (size_t)S > loo_partial_pairs_bound(N, S)) {
    set_error("dvae_sep_loo_logq: internal workspace bound violated (N %ld, S %ld, chunks %d)", N, S, chunks);
    return -3;
  }
  const unsigned sblocks = (unsigned)((S + 255) / 256);
  const dim3 grid(sblocks, (unsigned)chunks);
  hipLaunchKernelGGL(k_loo_prep, dim3((unsigned)((Npad + 255) / 256)), dim3(256), 0, st, mean, logvar, N, Npad, D, DP, rec);
  DVAE_CHECK_LAUNCH();
  switch (D <= DVAE_SEP_TEMPLATE_D ? DP : 0) {
    case 2: hipLaunchKernelGGL(k_loo_lse<2>, grid, dim3(256), 0, st, z, rec, D, S, chunk, part); break;
    case 4: hipLaunchKernelGGL(k_loo_lse<4>, grid, dim3(256), 0, st, z, rec, D, S, chunk, part); break;
    case 6: hipLaunchKernelGGL(k_loo_lse<6>, grid, dim3(256), 0, st, z, rec, D, S, chunk, part); break;
    case 8: hipLaunchKernelGGL(k_loo_lse<8>, grid, dim3(256), 0, st, z, rec, D, S, chunk, part); break;
    case 10: hipLaunchKernelGGL(k_loo_lse<10>, grid, dim3(256), 0, st, z, rec, D, S, chunk, part); break;
    case 12: hipLaunchKernelGGL(k_loo_lse<12>, grid, dim3(256), 0, st, z, rec, D, S, chunk, part); break;
    case 14: hipLaunchKernelGGL(k_loo_lse<14>, grid, dim3(256), 0, st, z, rec, D, S, chunk, part); break;
    case 16: hipLaunchKernelGGL(k_loo_lse<16>, grid, dim3(256), 0, st, z, rec, D, S, chunk, part); break;
    default: {
      const dim3 wide(sblocks, (unsigned)chunks, (unsigned)((D + 1 + DVAE_SEP_GROUP - 1) / DVAE_SEP_GROUP));
      hipLaunchKernelGGL(k_loo_lse_wide, wide, dim3(256), (size_t)D * 256 * sizeof(float), st, z, rec, D, S, chunk, part);
    }
  }
  DVAE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_loo_finish, dim3(sblocks, (unsigned)(D + 1)), dim3(256), 0, st, part, chunks, N, D, S, logq);
  DVAE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_loo_means, dim3((unsigned)(D + 1)), dim3(1024), 0, st, logq, S, H);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int dvae_sep_cond_terms(const float* eps, const float* logvar, const int64_t* rows, long N, int D, long S, double* H_cond_d,
                        void* stream) {
  DVAE_CHECK_ARG(eps && logvar && rows && H_cond_d);
  DVAE_CHECK_ARG(N > 0 && S > 0 && S <= (1L << 38));
  DVAE_CHECK_ARG(D >= 1 && D <= DVAE_SEP_MAX_D);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_sep_cond_terms, dim3((unsigned)D), dim3(1024), 0, st, eps, logvar, rows, D, S, H_cond_d);
  DVAE_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
