// libdvae_info_hip.so (include/dvae_info_hip.h): the two statistics of the [N, D] table of posterior means behind the discretised
// MIG (Locatello et al. 2019), modularity (Ridgeway & Mozer 2018) and the continuous-factor SAP score (Kumar et al. 2018):
// the centred moments of every (latent, factor) pair and the D x K family of joint histograms, over S selected rows.  The data
// set enumerates lat_sizes, so the factor values of a row are digits of its row number: v_k(r) = (r / stride_k) % lat_sizes[k].
//
// Moments.  DP consecutive lanes read the DP <= 64 consecutive floats of one row (DP = D padded to 4 / 16 / 64; D > 64 walks
// the row in pieces of 64), as the group statistics of factor_scores.hip do; lane dl of a row's DP lanes also divides out digit
// dl (and dl + DP) of the row number, the row's lanes exchange the digits by shuffle.  Every lane keeps min, max and the fp64
// sums of dx, dx^2 and dx dv_k with dx = x - x_0, dv = v - v_0 (the first selected row): one pass, the sums carry the spread of
// the column, not its offset.  A workgroup owns one chunk of rows and writes one record of partial sums (xor butterfly, then
// the waves in wave order); k_info_moments_finish adds the records in chunk order.  No atomics: the same bits every run.
//
// Histograms.  One workgroup per (chunk of rows, latent d), a lane per row: the bin is a count of edges <= x (edges in LDS, all
// lanes read the same word).  The data set is in factor order, so 64 consecutive rows share the value of every slow factor, and
// a disentangled latent puts them in one or two bins as well: per-lane adds would put a whole wave on one counter.  So a wave
// first asks, per factor, whether its rows share the value (one vote).  If any factor does, it builds its histogram over the bins
// -- one ballot + popcount per DISTINCT bin present, the count landing in the lane of that bin's number -- and adds that with at
// most n_bins adds on distinct counters; the other factors take one add per lane.  Counters live in LDS when one latent's
// n_bins * sum(lat_sizes) fit (DVAE_INFO_HIST_LDS_INTS) and are added to `counts` at the workgroup's end, else the same adds go
// to global memory.  Integer adds: any order gives the same counts.  k_info_zero clears `counts` first.
#include "../../include/dvae_info_hip.h"
#include "common.h"
#include "last_error.h"
#include "table_stats.h"

namespace dvae {

namespace {

#define INFO_T 256
#define INFO_KMAX DVAE_INFO_MAX_FACTORS

// (kept here: built on a helper shared with factor_irs.hip's load_factor, k_info_joint_hist compiled to other machine code)
// sizes (>= 1) and strides of the K factors, the same in every thread.  A stride that does not fit 32 bits saturates: row numbers
// are below 2^31, the digit is then 0.  Returns sum(lat_sizes), or -1 when a size is not positive.
struct Factors {
  unsigned size[INFO_KMAX], stride[INFO_KMAX];
};
__device__ __forceinline__ long load_factors(const int32_t* __restrict__ lat_sizes, int K, Factors* f) {
  long sum = 0;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < INFO_KMAX; ++k) {
    const int L = k < K ? lat_sizes[k] : 1;
    ok = ok && L >= 1;
    f->size[k] = L >= 1 ? (unsigned)L : 1u;
    if (k < K) sum += f->size[k];
  }
  unsigned long long s = 1;
#pragma unroll
  for (int k = INFO_KMAX - 1; k >= 0; --k) {
    f->stride[k] = (unsigned)s;
    if (k < K) s = lesser(s * f->size[k], 0xFFFFFFFFull);
  }
  return ok ? sum : -1;
}

// combination of v over the 256 / DP threads that share a dimension (same t % DP); every thread gets the same bits.  Fixed
// order: the xor butterfly inside a wave, then the waves in wave order.  EVERY thread of the workgroup calls.
struct OpSum { __device__ static double f(double a, double b) { return a + b; } };
struct OpMin { __device__ static double f(double a, double b) { return a < b ? a : b; } };
struct OpMax { __device__ static double f(double a, double b) { return a > b ? a : b; } };
template <int DP, class Op>
__device__ __forceinline__ double block_combine(double v, double* red, int t) {
#pragma unroll
  for (int o = 32; o >= DP; o >>= 1) v = Op::f(v, __shfl_xor(v, o, 64));
  __syncthreads();                                           // the previous call's reads of red are done
  if ((t & 63) < DP) red[(t >> 6) * 64 + (t & 63)] = v;
  __syncthreads();
  v = red[(t & 63) % DP];
#pragma unroll
  for (int w = 1; w < INFO_T / 64; ++w) v = Op::f(v, red[w * 64 + (t & 63) % DP]);
  return v;
}

// record of one chunk, in doubles: [D][4 + K] = min, max, sum dx, sum dx^2, sum dx dv_k;  then [K][2] = sum dv_k, sum dv_k^2
__host__ __device__ __forceinline__ long moments_record(int D, int K) { return (long)D * (4 + K) + 2L * K; }

template <int DP>
__global__ __launch_bounds__(INFO_T) void k_info_moments_part(const float* __restrict__ table, const int64_t* __restrict__ rows,
                                                              const int32_t* __restrict__ lat_sizes, int D, int K, long S, long chunk,
                                                              float* __restrict__ ws) {
  __shared__ double red[INFO_T];
  constexpr int NSUB = INFO_T / DP;
  const int t = threadIdx.x, sub = t / DP, dl = t % DP;
  const int group0 = (t & 63) - dl;                          // the first lane of this row's DP lanes
  Factors f;
  load_factors(lat_sizes, K, &f);
  const long c0 = blockIdx.x * chunk, c1 = lesser(S, c0 + chunk);
  const unsigned r0 = rows ? (unsigned)rows[0] : 0u;
  float* rec = ws + 2 * blockIdx.x * moments_record(D, K);
  // digit dl and digit dl + DP of a row number (DP >= 4, K <= 8: two per lane cover every factor)
  const int ka = dl < INFO_KMAX ? dl : 0, kb = dl + DP < INFO_KMAX ? dl + DP : 0;
  unsigned sa = 1, za = 1, sb = 1, zb = 1;
#pragma unroll
  for (int k = 0; k < INFO_KMAX; ++k) {
    if (k == ka) { sa = f.stride[k]; za = f.size[k]; }
    if (k == kb) { sb = f.stride[k]; zb = f.size[k]; }
  }
  const int va0 = (int)((r0 / sa) % za), vb0 = (int)((r0 / sb) % zb);
  for (int d0 = 0; d0 < D; d0 += DP) {
    const int d = d0 + dl;
    const bool on = d < D;                                   // the same for every thread that shares dl
    const float* col = table + (on ? d : 0);
    const double x0 = (double)col[(long)r0 * D];
    float mn = INFINITY, mx = -INFINITY;
    double s1 = 0., s2 = 0., fa1 = 0., fa2 = 0., fb1 = 0., fb2 = 0., c[INFO_KMAX];
#pragma unroll
    for (int k = 0; k < INFO_KMAX; ++k) c[k] = 0.;
    for (long base = c0; base < c1; base += NSUB) {          // the same trip count in every thread: the shuffles below are whole-wave
      const long l = base + sub;
      const bool valid = l < c1;
      const unsigned r = valid ? (rows ? (unsigned)rows[l] : (unsigned)l) : r0;
      const int dva = (int)((r / sa) % za) - va0, dvb = (int)((r / sb) % zb) - vb0;
      const float x = col[(long)r * D];
      const double dx = (double)x - x0;
      if (valid && on) {
        mn = fminf(mn, x);
        mx = fmaxf(mx, x);
        s1 += dx;
        s2 += dx * dx;
      }
      if (valid && d0 == 0) {                                // the factors' own sums: once, by the lane that divided the digit out
        fa1 += (double)dva; fa2 += (double)dva * (double)dva;
        fb1 += (double)dvb; fb2 += (double)dvb * (double)dvb;
      }
#pragma unroll
      for (int k = 0; k < INFO_KMAX; ++k) {
        if (k < K) {
          const int dv = __shfl(k < DP ? dva : dvb, group0 + k % DP, 64);
          if (valid && on) c[k] += dx * (double)dv;
        }
      }
    }
    const double bmn = block_combine<DP, OpMin>((double)mn, red, t), bmx = block_combine<DP, OpMax>((double)mx, red, t);
    s1 = block_combine<DP, OpSum>(s1, red, t);
    s2 = block_combine<DP, OpSum>(s2, red, t);
#pragma unroll
    for (int k = 0; k < INFO_KMAX; ++k)
      if (k < K) c[k] = block_combine<DP, OpSum>(c[k], red, t);
    if (on && sub == 0) {
      float* p = rec + 2L * d * (4 + K);
      put_f64(p, bmn); put_f64(p + 2, bmx); put_f64(p + 4, s1); put_f64(p + 6, s2);
#pragma unroll
      for (int k = 0; k < INFO_KMAX; ++k)
        if (k < K) put_f64(p + 8 + 2 * k, c[k]);
    }
    if (d0 == 0) {
      fa1 = block_combine<DP, OpSum>(fa1, red, t); fa2 = block_combine<DP, OpSum>(fa2, red, t);
      fb1 = block_combine<DP, OpSum>(fb1, red, t); fb2 = block_combine<DP, OpSum>(fb2, red, t);
      float* p = rec + 2L * D * (4 + K);
      if (sub == 0 && dl < K) { put_f64(p + 4 * dl, fa1); put_f64(p + 4 * dl + 2, fa2); }
      if (sub == 0 && dl + DP < K) { put_f64(p + 4 * (dl + DP), fb1); put_f64(p + 4 * (dl + DP) + 2, fb2); }
    }
  }
}

// one workgroup: the nb records added in chunk order into record nb, then the statistics from it
__global__ __launch_bounds__(INFO_T) void k_info_moments_finish(const float* __restrict__ table, const int64_t* __restrict__ rows,
                                                                const int32_t* __restrict__ lat_sizes, int D, int K, long S, int nb,
                                                                float* __restrict__ ws, float* __restrict__ col_min,
                                                                float* __restrict__ col_max, float* __restrict__ col_mean,
                                                                float* __restrict__ col_var, float* __restrict__ cov_zv,
                                                                float* __restrict__ factor_mean, float* __restrict__ factor_var) {
  const long rec = moments_record(D, K), col_part = (long)D * (4 + K);
  float* tot = ws + 2 * nb * rec;
  for (long i = threadIdx.x; i < rec; i += INFO_T) {
    const int q = i < col_part ? (int)(i % (4 + K)) : 2;
    double a = get_f64(ws + 2 * i);
    for (int b = 1; b < nb; ++b) {
      const double v = get_f64(ws + 2 * (b * rec + i));
      a = q == 0 ? (a < v ? a : v) : q == 1 ? (a > v ? a : v) : a + v;
    }
    put_f64(tot + 2 * i, a);
  }
  __syncthreads();
  Factors f;
  load_factors(lat_sizes, K, &f);
  const unsigned r0 = rows ? (unsigned)rows[0] : 0u;
  const double n = (double)S, n1 = S > 1 ? (double)(S - 1) : 1.;
  for (long i = threadIdx.x; i < (long)D * (K + 1) + K; i += INFO_T) {
    if (i < (long)D * (K + 1)) {
      const int d = (int)(i / (K + 1)), j = (int)(i % (K + 1));
      const float* p = tot + 2L * d * (4 + K);
      const double s1 = get_f64(p + 4);
      if (j == K) {
        const double s2 = get_f64(p + 6), var = (s2 - s1 * s1 / n) / n1;
        col_min[d] = (float)get_f64(p);
        col_max[d] = (float)get_f64(p + 2);
        col_mean[d] = (float)((double)table[(long)r0 * D + d] + s1 / n);
        col_var[d] = S > 1 && var > 0. ? (float)var : 0.f;
      } else {
        const double f1 = get_f64(tot + 2 * (col_part + 2 * j));
        cov_zv[(long)d * K + j] = S > 1 ? (float)((get_f64(p + 8 + 2 * j) - s1 * f1 / n) / n1) : 0.f;
      }
    } else {
      const int k = (int)(i - (long)D * (K + 1));
      unsigned stride = 1, size = 1;
#pragma unroll
      for (int kk = 0; kk < INFO_KMAX; ++kk)
        if (kk == k) { stride = f.stride[kk]; size = f.size[kk]; }
      const double f1 = get_f64(tot + 2 * (col_part + 2 * k)), f2 = get_f64(tot + 2 * (col_part + 2 * k + 1));
      const double var = (f2 - f1 * f1 / n) / n1;
      factor_mean[k] = (float)((double)((r0 / stride) % size) + f1 / n);
      factor_var[k] = S > 1 && var > 0. ? (float)var : 0.f;
    }
  }
}

__global__ __launch_bounds__(INFO_T) void k_info_zero(int32_t* __restrict__ p, long n) {
  zero_i32<INFO_T>(p, n);
}

template <bool LDS>
__global__ __launch_bounds__(INFO_T) void k_info_joint_hist(const float* __restrict__ table, const int64_t* __restrict__ rows,
                                                            const int32_t* __restrict__ lat_sizes, const float* __restrict__ edges,
                                                            int D, int K, long S, int n_bins, long sum_sizes, long chunk,
                                                            int32_t* __restrict__ counts) {
  __shared__ int h[LDS ? DVAE_INFO_HIST_LDS_INTS : 1];
  __shared__ float edge[DVAE_INFO_MAX_BINS];
  const int t = threadIdx.x, lane = t & 63, d = blockIdx.y;
  Factors f;
  if (load_factors(lat_sizes, K, &f) != sum_sizes) return;  // (the same in every thread) the caller's layout is not the device's
  const long tot = n_bins * sum_sizes;                       // the counters of one latent; LDS: at most DVAE_INFO_HIST_LDS_INTS
  long off[INFO_KMAX];                                       // where factor k's [n_bins, size_k] block starts among them
  long prefix = 0;
#pragma unroll
  for (int k = 0; k < INFO_KMAX; ++k) {
    off[k] = n_bins * prefix;
    if (k < K) prefix += f.size[k];
  }
  int32_t* gcnt = counts + d * tot;
  if (LDS)
    for (int i = t; i < (int)tot; i += INFO_T) h[i] = 0;
  if (t < n_bins) edge[t] = edges[(long)d * n_bins + t];
  __syncthreads();
  const long c0 = blockIdx.x * chunk, c1 = lesser(S, c0 + chunk);
  for (long base = c0 + (t - lane); base < c1; base += INFO_T) {   // wave-uniform: the votes and ballots below are whole-wave
    const long l = base + lane;
    const bool valid = l < c1;                               // (lane 0 always is)
    const unsigned r = valid ? (rows ? (unsigned)rows[l] : (unsigned)l) : 0u;
    const float x = table[(long)r * D + d];
    // (the count of edges stays in the kernel: as a helper shared with k_unsup_pair_hist it changed both kernels' machine code)
    int below = 0;
    for (int j = 0; j < n_bins; ++j) below += edge[j] <= x ? 1 : 0;
    const int b = min(max(below - 1, 0), n_bins - 1);
    int v[INFO_KMAX], v_first[INFO_KMAX];
    unsigned shared = 0;                                     // bit k: every row of the wave has the same value of factor k
#pragma unroll
    for (int k = 0; k < INFO_KMAX; ++k) {
      v[k] = v_first[k] = 0;
      if (k < K) {
        v[k] = (int)((r / f.stride[k]) % f.size[k]);
        v_first[k] = __builtin_amdgcn_readfirstlane(v[k]);
        if (__all(!valid || v[k] == v_first[k])) shared |= 1u << k;
      }
    }
    int in_my_bin = 0;                                       // lane j: how many rows of the wave fall into bin j (n_bins <= 64)
    if (shared) {
      unsigned long long rest = __ballot(valid);
      while (rest) {                                         // once per distinct bin present
        const int jb = __shfl(b, __ffsll(rest) - 1, 64);
        const unsigned long long m = __ballot(valid && b == jb);
        if (lane == jb) in_my_bin = __popcll(m);
        rest &= ~m;
      }
    }
#pragma unroll
    for (int k = 0; k < INFO_KMAX; ++k) {
      if (k < K) {
        const bool whole = (shared >> k) & 1u;
        const long at = off[k] + (long)(whole ? lane : b) * f.size[k] + (whole ? v_first[k] : v[k]);
        const int add = whole ? in_my_bin : (valid ? 1 : 0);
        if (add > 0) {
          if (LDS) atomicAdd(&h[at], add);
          else atomicAdd(&gcnt[at], add);
        }
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (int i = t; i < (int)tot; i += INFO_T) {
      const int cnt = h[i];
      if (cnt) atomicAdd(&gcnt[i], cnt);
    }
  }
}

static_assert(DVAE_INFO_ROW_LANES_NARROW == 4 && DVAE_INFO_ROW_LANES_MID == 16 && DVAE_INFO_ROW_LANES_WAVE == 64, "padded_width gives the row lanes");

bool sizes_ok(long N, int D, int K, long S) {
  return N > 0 && N <= 2000000000L && D > 0 && D <= 16384 && K > 0 && K <= DVAE_INFO_MAX_FACTORS && S > 0 && S <= 2000000000L;
}

}  // namespace
}  // namespace dvae

using namespace dvae;

extern "C" {

int dvae_info_version(void) { return DVAE_INFO_VERSION; }
const char* dvae_info_last_error(void) { return last_error(); }

size_t dvae_info_moments_ws_floats(long N, int D, int K, long S) {
  if (S <= 0) S = N;
  if (!sizes_ok(N, D, K, S)) return 0;
  long chunk;
  const int nb = chunks_of(S, DVAE_INFO_MOMENTS_BLOCK_ROWS, DVAE_INFO_MAX_BLOCKS, &chunk);
  return (size_t)(2 * (nb + 1) * moments_record(D, K));     // one record of doubles per chunk, and their total
}

size_t dvae_info_hist_ws_floats(long N, int D, int K, long S, int n_bins, long sum_sizes) {
  (void)N; (void)D; (void)K; (void)S; (void)n_bins; (void)sum_sizes;
  return 0;                                                    // the counters are integers: added where they lie
}

int dvae_info_moments(const float* table, const int64_t* rows, const int32_t* lat_sizes, long N, int D, int K, long S,
                      float* ws, float* col_min, float* col_max, float* col_mean, float* col_var, float* cov_zv,
                      float* factor_mean, float* factor_var, void* stream) {
  if (!rows) S = N;
  DVAE_CHECK_ARG(table && lat_sizes && ws && col_min && col_max && col_mean && col_var && cov_zv && factor_mean && factor_var);
  DVAE_CHECK_ARG(K <= DVAE_INFO_MAX_FACTORS);
  DVAE_CHECK_ARG(sizes_ok(N, D, K, S));
  hipStream_t st = (hipStream_t)stream;
  long chunk;
  const int nb = chunks_of(S, DVAE_INFO_MOMENTS_BLOCK_ROWS, DVAE_INFO_MAX_BLOCKS, &chunk);
  switch (padded_width(D)) {
    case DVAE_INFO_ROW_LANES_NARROW: hipLaunchKernelGGL((k_info_moments_part<DVAE_INFO_ROW_LANES_NARROW>), dim3(nb), dim3(INFO_T), 0, st, table, rows, lat_sizes, D, K, S, chunk, ws); break;
    case DVAE_INFO_ROW_LANES_MID: hipLaunchKernelGGL((k_info_moments_part<DVAE_INFO_ROW_LANES_MID>), dim3(nb), dim3(INFO_T), 0, st, table, rows, lat_sizes, D, K, S, chunk, ws); break;
    default: hipLaunchKernelGGL((k_info_moments_part<DVAE_INFO_ROW_LANES_WAVE>), dim3(nb), dim3(INFO_T), 0, st, table, rows, lat_sizes, D, K, S, chunk, ws);
  }
  DVAE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_info_moments_finish, dim3(1), dim3(INFO_T), 0, st, table, rows, lat_sizes, D, K, S, nb, ws, col_min, col_max,
                     col_mean, col_var, cov_zv, factor_mean, factor_var);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int dvae_info_joint_hist(const float* table, const int64_t* rows, const int32_t* lat_sizes, const float* edges, long N, int D,
                         int K, long S, int n_bins, long sum_sizes, float* ws, int32_t* counts, void* stream) {
  (void)ws;
  if (!rows) S = N;
  DVAE_CHECK_ARG(table && lat_sizes && edges && counts);
  DVAE_CHECK_ARG(K <= DVAE_INFO_MAX_FACTORS);
  DVAE_CHECK_ARG(n_bins >= 1 && n_bins <= DVAE_INFO_MAX_BINS);
  DVAE_CHECK_ARG(sizes_ok(N, D, K, S));
  DVAE_CHECK_ARG(sum_sizes >= K && sum_sizes <= 2000000000L && (double)D * n_bins * (double)sum_sizes <= 2147483647.);
  hipStream_t st = (hipStream_t)stream;
  const long tot = (long)n_bins * sum_sizes, all = (long)D * tot;
  hipLaunchKernelGGL(k_info_zero, dim3((unsigned)lesser((all + INFO_T - 1) / INFO_T, 1024L)), dim3(INFO_T), 0, st, counts, all);
  DVAE_CHECK_LAUNCH();
  long chunk;
  const int nb = chunks_of(S, DVAE_INFO_HIST_BLOCK_ROWS, DVAE_INFO_MAX_BLOCKS, &chunk);
  if (tot <= DVAE_INFO_HIST_LDS_INTS)
    hipLaunchKernelGGL((k_info_joint_hist<true>), dim3(nb, D), dim3(INFO_T), 0, st, table, rows, lat_sizes, edges, D, K, S, n_bins,
                       sum_sizes, chunk, counts);
  else
    hipLaunchKernelGGL((k_info_joint_hist<false>), dim3(nb, D), dim3(INFO_T), 0, st, table, rows, lat_sizes, edges, D, K, S, n_bins,
                       sum_sizes, chunk, counts);
  DVAE_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
