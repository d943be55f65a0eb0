// libdvae_mass_hip.so (include/dvae_mass_hip.h): the posterior mass table behind RMIG / JEMMIG (Do & Tran 2020), MIG-sup (Li et
// al. 2020) and DCIMIG (Sepliarskaia et al. 2019) -- q(z_d | x) of every selected row integrated over n_bins fixed bins and summed
// per value of every factor.  The data set enumerates lat_sizes, so the factor values of a row are digits of its row number:
// v_k(r) = (r / stride_k) % lat_sizes[k].  A COLUMN is one value of one factor: column sum(lat_sizes[:k]) + v, sum_sizes of them.
//
// k_mass_part.  One workgroup per (chunk of the selected rows, latent d, column group).  Lane l of wave w holds bin edge
// j = 63 w + l (e_0 = -inf and e_nb = +inf included) and, when l < 63, OWNS bin j: every accumulator [column, bin] has one owner
// thread, which adds the rows in their order -- no atomics, and no barrier inside the row walk, because a wave's last edge is
// evaluated again as the next wave's first.  A trip loads 64 rows, one per lane (row number, mean, sigma sqrt 2 and the columns
// of its K factor values), and walks them in order: the row's numbers are broadcast by v_readlane, every lane evaluates ONE erfc,
// the near tail erfc(|t_j|) / 2, and takes its upper neighbour's by a lane shift.  The mass of a bin is the difference of the two
// smaller tails (the header's rule); the far tail, needed next to the mean and in the end bins only, is 1 - (the near tail).  The
// accumulators of the group's columns live in LDS as [column][bin] (the lanes of a wave on consecutive doubles: no bank
// conflict whatever the factor sizes) and go to `ws` in that layout at the workgroup's end.
// k_mass_finish adds the chunks' partial tables in chunk order and writes `mass` in its [bin, value] layout.
#include "../../include/dvae_mass_hip.h"
#include "common.h"
#include "last_error.h"
#include "table_stats.h"

namespace dvae {

namespace {

#define MASS_KMAX DVAE_MASS_MAX_FACTORS
#define MASS_WB DVAE_MASS_WAVE_BINS
#define MASS_T_MAX ((DVAE_MASS_MAX_BINS + MASS_WB - 1) / MASS_WB * 64)
#define MASS_FT 256

static_assert(MASS_WB == 63 && DVAE_MASS_TRIP_ROWS == 64, "a lane per edge, the last one shared with the next wave; a lane per row of a trip");
static_assert(MASS_T_MAX <= 1024 && DVAE_MASS_MAX_BINS <= DVAE_MASS_LDS_DOUBLES, "one workgroup holds every edge and one column at the least");
static_assert(8L * DVAE_MASS_LDS_DOUBLES <= 160L * 1024, "the LDS of one CU");

// sizes (>= 1), saturating strides and first columns of the K factors, the same in every thread (factor_info.hip's load_factors
// with the columns added).  Returns sum(lat_sizes), or -1 when a size is not positive.
struct Factors {
  unsigned size[MASS_KMAX], stride[MASS_KMAX], first[MASS_KMAX];
};
__device__ __forceinline__ long load_factors(const int32_t* __restrict__ lat_sizes, int K, Factors* f) {
  long sum = 0;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < MASS_KMAX; ++k) {
    const int L = k < K ? lat_sizes[k] : 1;
    ok = ok && L >= 1;
    f->size[k] = L >= 1 ? (unsigned)L : 1u;
    f->first[k] = (unsigned)lesser(sum, 0x7FFFFFFFL);
    if (k < K) sum += f->size[k];
  }
  unsigned long long s = 1;
#pragma unroll
  for (int k = MASS_KMAX - 1; k >= 0; --k) {
    f->stride[k] = (unsigned)s;
    if (k < K) s = lesser(s * f->size[k], 0xFFFFFFFFull);
  }
  return ok ? sum : -1;
}

// lane i's value in every lane (i the same in every lane: v_readlane)
__device__ __forceinline__ int lane_i32(int v, int i) { return __builtin_amdgcn_readlane(v, i); }
__device__ __forceinline__ double lane_f64(double v, int i) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), i), __builtin_amdgcn_readlane(__double2loint(v), i));
}

__global__ __launch_bounds__(MASS_T_MAX) void k_mass_part(const float* __restrict__ mean, const float* __restrict__ logvar,
                                                          const int64_t* __restrict__ rows, const int32_t* __restrict__ lat_sizes,
                                                          const double* __restrict__ edges, int D, int K, long S, int n_bins,
                                                          long sum_sizes, long chunk, int group_cols, double* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) double acc[];          // [columns of this group][n_bins]
  const int t = threadIdx.x, lane = t & 63, d = blockIdx.y;
  const int j = (t >> 6) * MASS_WB + lane;                     // this lane's edge; bin j lies above it
  const bool owner = lane < MASS_WB && j < n_bins;
  Factors f;
  if (load_factors(lat_sizes, K, &f) != sum_sizes) return;    // (the same in every thread) k_mass_finish writes zeros
  const int col0 = blockIdx.z * group_cols, ncol = (int)lesser((long)group_cols, sum_sizes - col0);
  for (int i = t; i < ncol * n_bins; i += blockDim.x) acc[i] = 0.;
  __syncthreads();
  const bool finite_edge = j >= 1 && j < n_bins;             // e_0 = -inf: both tails of it are what lies below, 0; e_nb = +inf likewise
  const double e = finite_edge ? edges[j - 1] : 0.;
  const long c0 = blockIdx.x * chunk, c1 = lesser(S, c0 + chunk);
  for (long base = c0; base < c1; base += DVAE_MASS_TRIP_ROWS) {
    const long l = lesser(base + lane, c1 - 1);               // lanes past the chunk's end load its last row again and are not walked
    const unsigned r = rows ? (unsigned)rows[l] : (unsigned)l;
    const double mu_l = (double)mean[(long)r * D + d];
    const double den_l = exp(0.5 * (double)logvar[(long)r * D + d]) * 1.4142135623730951;    // sigma sqrt 2
    int col_l[MASS_KMAX];                                       // the row's column of factor k, counted from the group's first
#pragma unroll
    for (int k = 0; k < MASS_KMAX; ++k) col_l[k] = (int)(f.first[k] + (r / f.stride[k]) % f.size[k]) - col0;
    const int n = (int)lesser((long)DVAE_MASS_TRIP_ROWS, c1 - base);
    for (int i = 0; i < n; ++i) {
      const double tj = (e - lane_f64(mu_l, i)) / lane_f64(den_l, i);
      const int below = finite_edge ? (tj < 0. ? 1 : 0) : (j < 1 ? 1 : 0);   // the edge lies below the mean: its near tail is dn
      const double near = finite_edge ? 0.5 * erfc(fabs(tj)) : 0.;
      const double near_up = __shfl_down(near, 1, 64);          // of edge j + 1 (lane 63: its own; it owns no bin)
      const int below_up = __shfl_down(below, 1, 64);
      // t_j >= 0: up_j - up_{j+1};  t_j < 0: dn_{j+1} - dn_j, with dn_{j+1} = 1 - up_{j+1} where the mean lies in this bin
      const double q = below ? (below_up ? near_up : 1. - near_up) - near : near - near_up;
      if (owner) {
#pragma unroll
        for (int k = 0; k < MASS_KMAX; ++k) {
          if (k < K) {
            const int c = lane_i32(col_l[k], i);
            if ((unsigned)c < (unsigned)ncol) acc[c * n_bins + j] += q;
          }
        }
      }
    }
  }
  __syncthreads();
  double* part = ws + (((long)blockIdx.x * D + d) * sum_sizes + col0) * n_bins;
  for (int i = t; i < ncol * n_bins; i += blockDim.x) part[i] = acc[i];
}

// element i of one latent's [column][bin] table: the chunks' partial sums in chunk order, to its place in `mass`
__global__ __launch_bounds__(MASS_FT) void k_mass_finish(const int32_t* __restrict__ lat_sizes, int D, int K, int n_bins, long sum_sizes,
                                                         int chunks, const double* __restrict__ ws, double* __restrict__ mass) {
  const long tot = n_bins * sum_sizes, all = D * tot;
  const long i = blockIdx.x * (long)MASS_FT + threadIdx.x;
  if (i >= all) return;
  Factors f;
  if (load_factors(lat_sizes, K, &f) != sum_sizes) {          // the caller's layout is not the device's
    mass[i] = 0.;
    return;
  }
  double a = ws[i];
  for (int c = 1; c < chunks; ++c) a += ws[c * all + i];
  const long d = i / tot, col = (i % tot) / n_bins, b = i % n_bins;
  long first = 0, size = 1;
#pragma unroll
  for (int k = 0; k < MASS_KMAX; ++k)
    if (k < K && col >= f.first[k]) { first = f.first[k]; size = f.size[k]; }
  mass[d * tot + n_bins * first + b * size + (col - first)] = a;
}

bool sizes_ok(long N, int D, int K, long S, int n_bins, long sum_sizes) {
  return N > 0 && N <= 2000000000L && D > 0 && D <= 16384 && K > 0 && K <= DVAE_MASS_MAX_FACTORS && S > 0 && S <= 2000000000L &&
         n_bins >= 1 && n_bins <= DVAE_MASS_MAX_BINS && sum_sizes >= K && sum_sizes <= 2000000000L &&
         (double)D * n_bins * (double)sum_sizes <= 2147483647.;
}

// columns per group and the number of groups: as few groups as LDS allows, the columns spread evenly over them
int column_groups(int n_bins, long sum_sizes, int* group_cols) {
  const long fit = DVAE_MASS_LDS_DOUBLES / n_bins, groups = (sum_sizes + fit - 1) / fit;
  *group_cols = (int)((sum_sizes + groups - 1) / groups);
  return (int)((sum_sizes + *group_cols - 1) / *group_cols);
}

}  // namespace
}  // namespace dvae

using namespace dvae;

extern "C" {

int dvae_mass_version(void) { return DVAE_MASS_VERSION; }
const char* dvae_mass_last_error(void) { return last_error(); }

size_t dvae_mass_ws_doubles(long N, int D, int K, long S, int n_bins, long sum_sizes) {
  if (S <= 0) S = N;
  if (!sizes_ok(N, D, K, S, n_bins, sum_sizes)) return 0;
  long chunk;
  const int chunks = chunks_of(S, DVAE_MASS_BLOCK_ROWS, DVAE_MASS_MAX_CHUNKS, &chunk);
  return (size_t)chunks * (size_t)D * (size_t)n_bins * (size_t)sum_sizes;     // one [D][column][bin] table per chunk
}

int dvae_mass_joint(const float* mean, const float* logvar, const int64_t* rows, const int32_t* lat_sizes, const double* edges,
                    long N, int D, int K, long S, int n_bins, long sum_sizes, double* ws, double* mass, void* stream) {
  if (!rows) S = N;
  DVAE_CHECK_ARG(mean && logvar && lat_sizes && ws && mass);
  DVAE_CHECK_ARG(K >= 1 && K <= DVAE_MASS_MAX_FACTORS);
  DVAE_CHECK_ARG(n_bins >= 1 && n_bins <= DVAE_MASS_MAX_BINS);
  DVAE_CHECK_ARG(edges || n_bins == 1);
  DVAE_CHECK_ARG(sizes_ok(N, D, K, S, n_bins, sum_sizes));
  int group_cols;
  const int groups = column_groups(n_bins, sum_sizes, &group_cols);
  DVAE_CHECK_ARG(groups <= 65535);
  hipStream_t st = (hipStream_t)stream;
  long chunk;
  const int chunks = chunks_of(S, DVAE_MASS_BLOCK_ROWS, DVAE_MASS_MAX_CHUNKS, &chunk);
  const int threads = (n_bins + MASS_WB - 1) / MASS_WB * 64;
  const size_t lds = 8 * (size_t)group_cols * n_bins;
  static DeviceOnce attr;
  if (attr.first()) (void)hipFuncSetAttribute((const void*)k_mass_part, hipFuncAttributeMaxDynamicSharedMemorySize, 8 * DVAE_MASS_LDS_DOUBLES);
  hipLaunchKernelGGL(k_mass_part, dim3(chunks, D, groups), dim3(threads), lds, st, mean, logvar, rows, lat_sizes, edges, D, K, S, n_bins,
                     sum_sizes, chunk, group_cols, ws);
  DVAE_CHECK_LAUNCH();
  const long all = (long)D * n_bins * sum_sizes;
  hipLaunchKernelGGL(k_mass_finish, dim3((unsigned)((all + MASS_FT - 1) / MASS_FT)), dim3(MASS_FT), 0, st, lat_sizes, D, K, n_bins, sum_sizes,
                     chunks, ws, mass);
  DVAE_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
