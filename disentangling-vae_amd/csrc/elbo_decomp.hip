// libdvae_eval_hip.so (include/dvae_eval_hip.h): the data-set level ELBO decomposition of Chen et al. 2018 (beta-TCVAE, sec. 3)
//     KL term = I[z;n] + TC[z] + sum_d KL[q(z_d) || p(z_d)]
// estimated on S samples z_s ~ q(z|x_n(s)) against the aggregate posterior q(z) = 1/N sum_n q(z|x_n) of the whole data set.
// The marginal entropies H[z_d] come from dvae_latent_entropy (metrics.hip, the other library); what is computed here is the
// JOINT log-density
//     log q(z_s) = logsumexp_{n<N} sum_{d<D} log N(z_sd; mu_nd, exp(logvar_nd)) - log N
// -- S x N x D (5.4e11 (sample, data point) pairs for dSprites with S = N) with the sum over d INSIDE the logsumexp -- and the
// two per-sample terms that need only the sample's own row (log q(z_s | x_n(s)), log p(z_s)).
//
// Decomposition of the joint kernel: thread = one sample s with z_s[0..D) in registers, workgroup = 256 consecutive samples,
// gridDim.y = chunks of the data set.  Per data point ONE contiguous record {mu[DP], exp(-logvar)[DP], c = sum_d -0.5 (log 2pi +
// logvar_d)} (n-major, prepared once): it is wave-uniform in the main loop, so it arrives through scalar loads and feeds the
// VALU as scalar operands -- 3 VALU operations per (s, n, d) (subtract, square, multiply-add) and one v_exp_f32 per 8 D of them
// (online logsumexp, one rescale per 8 data points).  D is padded to DP in {4, 8, 12, 16}: padding has iv = 0, mu = 0, z = 0 and
// contributes exactly 0; the table is padded to whole chunks with records of density -inf (c = -inf), so the main loop has no
// tail.  Chunk partials (max, sum) are merged in chunk order; every sum has a fixed order (no atomics).
//
// NOT a GEMM on the matrix cores, on purpose: expanding (z - mu)^2 iv into z^2 iv - 2 z mu iv + mu^2 iv turns the contraction
// over d into a matrix product, but with the sharp posteriors of a trained model (iv ~ e^8 .. e^10) the three terms are 1e4
// times larger than their sum and cancel catastrophically in fp32: the dominant densities -- z a fraction of a standard deviation
// from mu -- would come out with absolute errors of order 1e-3 .. 1 in the exponent.  The difference is formed first.
#include <float.h>
#include "../../include/dvae_eval_hip.h"
#include "common.h"
#include "last_error.h"

namespace dvae {

namespace {

#define JOINT_TARGET_WGS 2048          // workgroups that fill the device: 256 CUs x 8 (4 waves each)
#define JOINT_WIDE_LDS_D 48            // run-time-D kernel: z of a workgroup in LDS up to this D (48 KB), re-read from memory above

// record of data point n at rec + n * (2 DP + 1): mu[0..DP), iv[0..DP), c.  Rows n >= N (padding up to whole chunks): c = -inf.
__global__ __launch_bounds__(256) void k_joint_prep(const float* __restrict__ mu, const float* __restrict__ lv, long N, long Npad,
                                                    int D, int DP, float* __restrict__ rec) {
  const long n = blockIdx.x * 256L + threadIdx.x;
  if (n >= Npad) return;
  float* r = rec + n * (2 * DP + 1);
  float c = 0.f;
  for (int d = 0; d < DP; ++d) {
    const bool real = n < N && d < D;
    const float l = real ? lv[n * D + d] : 0.f;
    r[d] = real ? mu[n * D + d] : 0.f;
    r[DP + d] = real ? expf(-l) : 0.f;
    if (real) c += gauss_c(l);
  }
  r[2 * DP] = n < N ? c : -INFINITY;
}

// part[c][0][s] = running max, part[c][1][s] = sum of exp(density - max) over the chunk's data points
template <int DP>
__global__ __launch_bounds__(256) void k_joint_lse(const float* __restrict__ z, const float* __restrict__ rec, int D, long S,
                                                   int chunk, float* __restrict__ part) {
  constexpr int R = 2 * DP + 1;
  const long s = blockIdx.x * 256L + threadIdx.x;
  float zr[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) zr[d] = (s < S && d < D) ? z[s * D + d] : 0.f;
  const float* r = rec + (long)blockIdx.y * chunk * R;        // wave-uniform: scalar loads
  float m = -INFINITY, acc = 0.f;
  for (int i = 0; i < chunk; i += 8, r += 8 * R) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float* q = r + u * R;
      float a = 0.f;
#pragma unroll
      for (int d = 0; d < DP; ++d) {
        const float diff = zr[d] - q[d];
        a += diff * diff * q[DP + d];                         // log_density_gaussian, utils/math.py:48-50, summed over d in order
      }
      const float c = q[2 * DP];
      v[u] = c > -INFINITY ? c - 0.5f * a : -INFINITY;        // padding record: -inf whatever z is (inf * iv = NaN for iv = 0)
    }
    lse_fold8(v, m, acc);
  }
  if (s < S) {
    float* p = part + (long)blockIdx.y * 2 * S;
    p[s] = m;
    p[S + s] = acc;
  }
}

// D > 16: the same loop with a run-time D (record stride 2 D + 1).  z of the workgroup's samples sits in LDS as [D][256] (a
// thread reads its own column only: conflict-free, no barrier) when use_lds, else every thread re-reads its row from memory.
__global__ __launch_bounds__(256) void k_joint_lse_wide(const float* __restrict__ z, const float* __restrict__ rec, int D, long S,
                                                        int chunk, int use_lds, float* __restrict__ part) {
  extern __shared__ float zl[];
  const int R = 2 * D + 1;
  const long s = blockIdx.x * 256L + threadIdx.x;
  const float* zg = z + (s < S ? s : S - 1) * D;              // (threads past S compute a copy of the last sample, unwritten)
  if (use_lds)
    for (int d = 0; d < D; ++d) zl[d * 256 + threadIdx.x] = zg[d];
  const float* r = rec + (long)blockIdx.y * chunk * R;
  float m = -INFINITY, acc = 0.f;
  for (int i = 0; i < chunk; i += 8, r += 8 * R) {
    float v[8];
#pragma unroll 2
    for (int u = 0; u < 8; ++u) {
      const float* q = r + u * R;
      float a = 0.f;
      for (int d = 0; d < D; ++d) {
        const float diff = (use_lds ? zl[d * 256 + threadIdx.x] : zg[d]) - q[d];
        a += diff * diff * q[D + d];
      }
      const float c = q[2 * D];
      v[u] = c > -INFINITY ? c - 0.5f * a : -INFINITY;        // padding record: see k_joint_lse
    }
    lse_fold8(v, m, acc);
  }
  if (s < S) {
    float* p = part + (long)blockIdx.y * 2 * S;
    p[s] = m;
    p[S + s] = acc;
  }
}

// merge the chunk partials of every sample in chunk order: logqz[s] = logsumexp_n - log N
__global__ __launch_bounds__(256) void k_joint_finish(const float* __restrict__ part, int chunks, long N, long S,
                                                      float* __restrict__ logqz) {
  const long s = blockIdx.x * 256L + threadIdx.x;
  if (s >= S) return;
  float m = -INFINITY, acc = 0.f;
  for (int c = 0; c < chunks; ++c) {
    const float m2 = part[(long)c * 2 * S + s], a2 = part[(long)c * 2 * S + S + s];
    m = lse_merge(m, acc, m2, a2);
  }
  logqz[s] = m + logf(acc) - logf((float)N);                  // (m = -inf, acc = 0: -inf)
}

// thread = one sample: the two terms that need only its own row
__global__ __launch_bounds__(256) void k_sample_terms(const float* __restrict__ z, const float* __restrict__ eps,
                                                      const float* __restrict__ lv, const int64_t* __restrict__ rows, int D, long S,
                                                      float* __restrict__ logqz_condx, float* __restrict__ logpz) {
  const long s = blockIdx.x * 256L + threadIdx.x;
  if (s >= S) return;
  const float* l = lv + rows[s] * D;
  float qc = 0.f, pz = 0.f;
  for (int d = 0; d < D; ++d) {
    const float e = eps[s * D + d], zz = z[s * D + d];
    qc += gauss_c(l[d]) - 0.5f * (e * e);
    pz += -0.5f * LOG2PI - 0.5f * (zz * zz);
  }
  logqz_condx[s] = qc;
  logpz[s] = pz;
}

// out[b] = scale / S * sum_s src_b[s], b = blockIdx.x in {0, 1}: one workgroup per array, a fixed summation order
__global__ __launch_bounds__(1024) void k_eval_means(const float* __restrict__ a, const float* __restrict__ b, long S, float scale,
                                                     float* __restrict__ out) {
  __shared__ float red[16];
  const float* src = blockIdx.x == 0 ? a : b;
  float t = 0.f;
  for (long s = threadIdx.x; s < S; s += 1024) t += src[s];
  t = wave_sum(t);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int w = 0; w < 16; ++w) tot += red[w];
    out[blockIdx.x] = scale * tot / (float)S;
  }
}

int padded_dim(int D) { return D <= 4 ? 4 : D <= 8 ? 8 : D <= 12 ? 12 : D <= 16 ? 16 : D; }

long chunks_of_data(long N) {
  const long c = (N + DVAE_EVAL_JOINT_CHUNK - 1) / DVAE_EVAL_JOINT_CHUNK;
  return c < 1 ? 1 : (c > DVAE_EVAL_JOINT_MAX_CHUNKS ? DVAE_EVAL_JOINT_MAX_CHUNKS : c);
}

// chunks of at least DVAE_EVAL_JOINT_CHUNK data points, and no more of them than it takes to fill the device next to the
// sample blocks (the partials cost chunks * S * 2 floats)
int joint_chunks(long N, long S) {
  const long sblocks = (S + 255) / 256;
  const long by_s = JOINT_TARGET_WGS / sblocks < 1 ? 1 : JOINT_TARGET_WGS / sblocks;
  const long c = chunks_of_data(N);
  return (int)(c < by_s ? c : by_s);
}

// bounds of the two workspace parts that are non-decreasing in N and in S (the chunk count itself falls as S grows):
// table rows <= N + 8 chunks (chunk length rounded up to 8);  chunks * S <= min(chunks_of_data * S, max(S, 256 * target))
size_t table_rows_bound(long N) { return (size_t)N + 8 * (size_t)chunks_of_data(N); }
size_t partial_pairs_bound(long N, long S) {
  const size_t a = (size_t)chunks_of_data(N) * (size_t)S;
  const size_t b = (size_t)S > (size_t)JOINT_TARGET_WGS * 256 ? (size_t)S : (size_t)JOINT_TARGET_WGS * 256;
  return a < b ? a : b;
}

}  // namespace
}  // namespace dvae

using namespace dvae;

extern "C" {

int dvae_eval_version(void) { return DVAE_EVAL_VERSION; }
const char* dvae_eval_last_error(void) { return last_error(); }

size_t dvae_eval_joint_logq_ws_floats(long N, int D, long S) {
  if (N <= 0 || D <= 0 || S <= 0) return 0;
  return table_rows_bound(N) * (size_t)(2 * padded_dim(D) + 1) + 2 * partial_pairs_bound(N, S);
}

int dvae_eval_joint_logq(const float* z, const float* mean, const float* logvar, long N, int D, long S, float* ws, float* logqz,
                         float* H_joint, void* stream) {
  DVAE_CHECK_ARG(z && mean && logvar && ws && logqz && H_joint);
  DVAE_CHECK_ARG(N > 0 && N <= 2000000000L && D > 0 && D <= 16384 && S > 0 && S <= (1L << 38));
  hipStream_t st = (hipStream_t)stream;
  const int DP = padded_dim(D);
  const int chunks = joint_chunks(N, S);
  const int chunk = (int)(((N + chunks - 1) / chunks + 7) / 8 * 8);
  const long Npad = (long)chunks * chunk;
  float* rec = ws;
  float* part = ws + table_rows_bound(N) * (size_t)(2 * DP + 1);
  if ((size_t)Npad > table_rows_bound(N) || (size_t)chunks * (size_t)S > partial_pairs_bound(N, S)) {
    set_error("dvae_eval_joint_logq: internal workspace bound violated (N %ld, S %ld, chunks %d)", N, S, chunks);
    return -3;
  }
  const dim3 grid((unsigned)((S + 255) / 256), (unsigned)chunks);
  hipLaunchKernelGGL(k_joint_prep, dim3((unsigned)((Npad + 255) / 256)), dim3(256), 0, st, mean, logvar, N, Npad, D, DP, rec);
  DVAE_CHECK_LAUNCH();
  switch (DP) {
    case 4: hipLaunchKernelGGL(k_joint_lse<4>, grid, dim3(256), 0, st, z, rec, D, S, chunk, part); break;
    case 8: hipLaunchKernelGGL(k_joint_lse<8>, grid, dim3(256), 0, st, z, rec, D, S, chunk, part); break;
    case 12: hipLaunchKernelGGL(k_joint_lse<12>, grid, dim3(256), 0, st, z, rec, D, S, chunk, part); break;
    case 16: hipLaunchKernelGGL(k_joint_lse<16>, grid, dim3(256), 0, st, z, rec, D, S, chunk, part); break;
    default: {
      const int use_lds = D <= JOINT_WIDE_LDS_D;
      hipLaunchKernelGGL(k_joint_lse_wide, grid, dim3(256), use_lds ? (size_t)D * 256 * sizeof(float) : 0, st, z, rec, D, S, chunk,
                         use_lds, part);
    }
  }
  DVAE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_joint_finish, dim3(grid.x), dim3(256), 0, st, part, chunks, N, S, logqz);
  DVAE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_eval_means, dim3(1), dim3(1024), 0, st, logqz, logqz, S, -1.f, H_joint);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int dvae_eval_sample_terms(const float* z, const float* eps, const float* logvar, const int64_t* rows, long N, int D, long S,
                           float* logqz_condx, float* logpz, float* means, void* stream) {
  DVAE_CHECK_ARG(z && eps && logvar && rows && logqz_condx && logpz && means);
  DVAE_CHECK_ARG(N > 0 && D > 0 && S > 0 && S <= (1L << 38));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_sample_terms, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, z, eps, logvar, rows, D, S, logqz_condx,
                     logpz);
  DVAE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_eval_means, dim3(2), dim3(1024), 0, st, logqz_condx, logpz, S, 1.f, means);
  DVAE_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
