// libdvae_score_hip.so (include/dvae_score_hip.h): the batched statistics behind the FactorVAE score (Kim & Mnih 2018, sec. 4)
// and the beta-VAE score (Higgins et al. 2017, sec. 3).  Both scores gather V groups of L rows from the [N, D] table of
// posterior means (V = 10 000 + 5 000, L = 64 by default; one group of 10 000 rows for the global variance) and reduce each
// group per latent dimension: the unbiased variance (FactorVAE) or the mean absolute difference of two gathered rows
// (beta-VAE).  The FactorVAE score then takes the arg-min dimension of every group and counts (factor, dimension) votes.
//
// Decomposition of the two group statistics: DP consecutive lanes read the DP <= 64 consecutive floats of one gathered row
// (DP = D padded to 4 / 16 / 64; D > 64 walks the row in pieces of 64), so a wave instruction fetches 64 / DP whole rows and
// every fetched sector is used; the lanes that share a dimension each sum their rows in row order and are then combined by
// an xor butterfly (which gives every lane the same bits).  Two launch shapes on L (DVAE_SCORE_WAVE_MAX_L):
//   wave  (T = 64):  one group per wave, four groups per workgroup, no barrier, no LDS;
//   block (T = 256): one group per workgroup, the four wave results combined through LDS in wave order.
// Rows of the table are aligned to 4 bytes only (D = 10: 40-byte rows): every load is one float.
//
// The variance is taken around the group's mean -- mean first, squared deviations second, the rows re-read from cache --
// and both passes work on x - x_0 (the group's first row): the sums then carry the spread of the group, not its offset.
#include "../../include/dvae_score_hip.h"
#include "common.h"
#include "last_error.h"
#include "table_stats.h"

namespace dvae {

namespace {

#define SCORE_GROUPS_PER_WG 4          // wave shape: 256 threads = 4 waves = 4 groups

// sum of v over the T / DP threads of a group that share a dimension (same t % DP); every thread gets the same bits.
// Fixed order: the xor butterfly inside a wave, then the waves in wave order.  T == 256: EVERY thread of the workgroup calls.
template <int DP, int T>
__device__ __forceinline__ float group_sum(float v, float* red, int t) {
#pragma unroll
  for (int o = 32; o >= DP; o >>= 1) v += __shfl_xor(v, o, 64);
  if (T > 64) {
    __syncthreads();                                         // the previous call's reads of red are done
    if ((t & 63) < DP) red[(t >> 6) * 64 + (t & 63)] = v;
    __syncthreads();
    v = 0.f;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) v += red[w * 64 + (t & 63) % DP];
  }
  return v;
}

// which group and which thread of it: wave shape -> (4 blockIdx + wave, lane), block shape -> (blockIdx, threadIdx)
template <int T>
__device__ __forceinline__ long group_of(int* t) {
  *t = T == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
  return T == 64 ? (long)blockIdx.x * SCORE_GROUPS_PER_WG + (threadIdx.x >> 6) : (long)blockIdx.x;
}

template <int DP, int T>
__global__ __launch_bounds__(256) void k_group_var(const float* __restrict__ table, const int64_t* __restrict__ rows, int D, long V,
                                                   long L, const float* __restrict__ inv_scale, float* __restrict__ out) {
  __shared__ float red[256];
  constexpr int NSUB = T / DP;
  int t;
  const long v = group_of<T>(&t);
  if (v >= V) return;                                        // wave shape only, wave-uniform (block shape: grid = V)
  const int sub = t / DP, dl = t % DP;
  const int64_t* r = rows + v * L;
  for (int d0 = 0; d0 < D; d0 += DP) {
    const int d = d0 + dl;
    const bool on = d < D;                                   // the same for every thread that shares dl
    const float* col = table + (on ? d : 0);
    const float x0 = col[r[0] * D];
    float s = 0.f;
    if (on) {
#pragma unroll 4
      for (long l = sub; l < L; l += NSUB) s += col[r[l] * D] - x0;
    }
    const float m = group_sum<DP, T>(s, red, t) / (float)L;  // mean of x - x0
    float q = 0.f;
    if (on) {
#pragma unroll 4
      for (long l = sub; l < L; l += NSUB) {
        const float dev = (col[r[l] * D] - x0) - m;
        q += dev * dev;
      }
    }
    q = group_sum<DP, T>(q, red, t);
    if (on && sub == 0) {
      const float var = q / (float)(L - 1);
      out[v * D + d] = inv_scale ? var * inv_scale[d] : var;
    }
  }
}

template <int DP, int T>
__global__ __launch_bounds__(256) void k_pair_absdiff(const float* __restrict__ table, const int64_t* __restrict__ rows_a,
                                                      const int64_t* __restrict__ rows_b, int D, long V, long L,
                                                      float* __restrict__ out) {
  __shared__ float red[256];
  constexpr int NSUB = T / DP;
  int t;
  const long v = group_of<T>(&t);
  if (v >= V) return;
  const int sub = t / DP, dl = t % DP;
  const int64_t* ra = rows_a + v * L;
  const int64_t* rb = rows_b + v * L;
  for (int d0 = 0; d0 < D; d0 += DP) {
    const int d = d0 + dl;
    const bool on = d < D;
    const float* col = table + (on ? d : 0);
    float s = 0.f;
    if (on) {
#pragma unroll 4
      for (long l = sub; l < L; l += NSUB) s += fabsf(col[ra[l] * D] - col[rb[l] * D]);
    }
    s = group_sum<DP, T>(s, red, t);
    if (on && sub == 0) out[v * D + d] = s / (float)L;
  }
}

// thread = one group: the active dimension with the smallest statistic, the lowest index on ties, never a NaN
__global__ __launch_bounds__(256) void k_vote_argmin(const float* __restrict__ stat, const int32_t* __restrict__ active, long V, int D,
                                                     int32_t* __restrict__ argmin) {
  const long v = blockIdx.x * 256L + threadIdx.x;
  if (v >= V) return;
  const float* s = stat + v * D;
  int best = -1;
  float bv = 0.f;
  for (int d = 0; d < D; ++d) {
    const float x = s[d];
    if (active[d] != 0 && x == x && (best < 0 || x < bv)) { best = d; bv = x; }
  }
  argmin[v] = best;
}

// K * D <= DVAE_SCORE_VOTE_LDS_BINS counters in LDS, one workgroup: integer adds (any order gives the same counts)
__global__ __launch_bounds__(1024) void k_vote_count_lds(const int32_t* __restrict__ argmin, const int32_t* __restrict__ factor, long V,
                                                         int D, int K, int32_t* __restrict__ votes) {
  const int bins = K * D;
  __shared__ int cnt[DVAE_SCORE_VOTE_LDS_BINS];
  for (int i = threadIdx.x; i < bins; i += 1024) cnt[i] = 0;
  __syncthreads();
  for (long v = threadIdx.x; v < V; v += 1024) {
    const int d = argmin[v], k = factor[v];
    if (d >= 0 && (unsigned)k < (unsigned)K) atomicAdd(&cnt[k * D + d], 1);   // (a factor outside [0, K) has no counter)
  }
  __syncthreads();
  for (int i = threadIdx.x; i < bins; i += 1024) votes[i] = cnt[i];
}

// more counters than fit LDS: thread = one counter (k, d), walking the groups in order
__global__ __launch_bounds__(256) void k_vote_count_wide(const int32_t* __restrict__ argmin, const int32_t* __restrict__ factor, long V,
                                                         int D, long bins, int32_t* __restrict__ votes) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= bins) return;
  const int k = (int)(i / D), d = (int)(i % D);
  int c = 0;
  for (long v = 0; v < V; ++v) c += (argmin[v] == d && factor[v] == k) ? 1 : 0;
  votes[i] = c;
}

#define SCORE_LAUNCH(kern, DP, ...)                                                                                       \
  do {                                                                                                                    \
    if (L <= DVAE_SCORE_WAVE_MAX_L)                                                                                       \
      hipLaunchKernelGGL((kern<DP, 64>), dim3((unsigned)((V + SCORE_GROUPS_PER_WG - 1) / SCORE_GROUPS_PER_WG)), dim3(256), \
                         0, st, __VA_ARGS__);                                                                             \
    else                                                                                                                  \
      hipLaunchKernelGGL((kern<DP, 256>), dim3((unsigned)V), dim3(256), 0, st, __VA_ARGS__);                              \
  } while (0)

#define SCORE_DISPATCH(kern, ...)                                \
  switch (padded_width(D)) {                                       \
    case 4: SCORE_LAUNCH(kern, 4, __VA_ARGS__); break;           \
    case 16: SCORE_LAUNCH(kern, 16, __VA_ARGS__); break;         \
    default: SCORE_LAUNCH(kern, 64, __VA_ARGS__);                \
  }

}  // namespace
}  // namespace dvae

using namespace dvae;

extern "C" {

int dvae_score_version(void) { return DVAE_SCORE_VERSION; }
const char* dvae_score_last_error(void) { return last_error(); }

size_t dvae_score_group_var_ws_floats(long N, int D, long V, long L) {
  (void)N; (void)D; (void)V; (void)L;
  return 0;                                                    // both launch shapes reduce a group inside one workgroup
}

int dvae_score_group_var(const float* table, const int64_t* rows, long N, int D, long V, long L, const float* inv_scale,
                         float* ws, float* out, void* stream) {
  (void)ws;
  DVAE_CHECK_ARG(table && rows && out);
  DVAE_CHECK_ARG(N > 0 && N <= 2000000000L && D > 0 && D <= 16384 && V > 0 && V <= (1L << 30) && L >= 2 && L <= (1L << 30));
  hipStream_t st = (hipStream_t)stream;
  SCORE_DISPATCH(k_group_var, table, rows, D, V, L, inv_scale, out);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int dvae_score_pair_absdiff(const float* table, const int64_t* rows_a, const int64_t* rows_b, long N, int D, long V, long L,
                            float* out, void* stream) {
  DVAE_CHECK_ARG(table && rows_a && rows_b && out);
  DVAE_CHECK_ARG(N > 0 && N <= 2000000000L && D > 0 && D <= 16384 && V > 0 && V <= (1L << 30) && L >= 1 && L <= (1L << 30));
  hipStream_t st = (hipStream_t)stream;
  SCORE_DISPATCH(k_pair_absdiff, table, rows_a, rows_b, D, V, L, out);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int dvae_score_vote(const float* stat, const int32_t* factor, const int32_t* active, long V, int D, int K, int32_t* argmin,
                    int32_t* votes, void* stream) {
  DVAE_CHECK_ARG(stat && factor && active && argmin && votes);
  DVAE_CHECK_ARG(V > 0 && V <= (1L << 38) && D > 0 && D <= 16384 && K > 0 && K <= 16384);
  hipStream_t st = (hipStream_t)stream;
  const long bins = (long)K * D;
  hipLaunchKernelGGL(k_vote_argmin, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, st, stat, active, V, D, argmin);
  DVAE_CHECK_LAUNCH();
  if (bins <= DVAE_SCORE_VOTE_LDS_BINS)
    hipLaunchKernelGGL(k_vote_count_lds, dim3(1), dim3(1024), 0, st, argmin, factor, V, D, K, votes);
  else
    hipLaunchKernelGGL(k_vote_count_wide, dim3((unsigned)((bins + 255) / 256)), dim3(256), 0, st, argmin, factor, V, D, bins, votes);
  DVAE_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
