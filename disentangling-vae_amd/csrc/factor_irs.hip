// libdvae_irs_hip.so (include/dvae_irs_hip.h): the two statistics of the [N, D] table of posterior means behind the interventional
// robustness score (Suter et al. 2019): the mean of every latent over every group of selected rows that share a (binned) factor
// value, and exact order statistics of the absolute deviations from a given centre per group.  The data set enumerates lat_sizes,
// so the group of a row is index arithmetic on its row number: g_k(r) = group_of_value[k][(r / stride_k) % lat_sizes[k]].  A
// chunked scan of the selected rows therefore serves rows = NULL and a selection alike; the table is never copied or sorted.
// Slot 0 of the group index space ("all selected rows") is handled as factor number 0 with one group, factor k as number k + 1.
//
// Means.  One workgroup per (chunk of rows, factor).  It stages tiles of 256 rows x at most 16 columns and the rows' group ids in
// LDS; one owner lane per (group, column) slot then adds, in row order, the fp64 x - x_0 of its group's rows (a select, no
// branch), and counts them.  Every workgroup writes one record of partial sums; k_irs_means_finish adds the records in chunk
// order.  No atomics: the same bits every run.
//
// Selection.  dev = |x - c| is never negative, so the deviations order like their bit patterns: a radix select, most significant
// byte first.  Per pass, one workgroup per (chunk, latent, factor, slice of at most 40 groups) counts the digit of every row whose
// higher digits equal the current prefix of its group into a [groups, 256] histogram in LDS -- the first few distinct
// (group, digit) keys of a wave by one ballot and one add each, the rest one add per lane -- and merges it into global integer
// counters.  k_irs_select_walk (one wave per (group, latent) pair) then finds the bin that holds the rank, extends the prefix,
// reduces the rank and clears the counters.  After the fourth pass the prefix IS the rank-th smallest deviation, and the walk knows
// how many deviations are <= it.  One more pass takes the largest deviation (integer max) and the smallest one above the prefix
// (integer min) per group; k_irs_select_finish picks stat_hi between the two.  Integer atomics only: any order gives the same bits.
#include "../../include/dvae_irs_hip.h"
#include "common.h"
#include "last_error.h"
#include "table_stats.h"

namespace dvae {

namespace {

#define IRS_T 256
#define IRS_KMAX DVAE_IRS_MAX_FACTORS
#define IRS_DC DVAE_IRS_MEANS_COLS
#define IRS_SLOTS (DVAE_IRS_MAX_GROUPS * IRS_DC / IRS_T)      // (group, column) slots one thread can own
#define IRS_LG DVAE_IRS_SELECT_LDS_GROUPS
#define IRS_AGG 4                                            // distinct keys of a wave that are added by ballot
#define IRS_NONE 0xFFFFFFFFu

// What one workgroup needs of the layout for ITS factor number j (0: "all selected rows", j >= 1: factor j - 1); the same in every
// thread.  ok: lat_sizes / n_groups agree with what the caller said of them (sum_sizes, total_groups, max_groups).  (The sizes and
// strides are formed here as in factor_info.hip's load_factors: built on one shared helper, five kernels compiled to other machine code.)
struct Factor {
  unsigned size, stride;  // value of a row: (r / stride) % size
  int voff;               // where the factor's values start in group_of_value
  int gbase, G;           // its groups' first slot and their number
  bool ok;
};
__device__ __forceinline__ Factor load_factor(const int32_t* __restrict__ lat_sizes, const int32_t* __restrict__ n_groups, int K,
                                              long sum_sizes, int total_groups, int max_groups, int j) {
  Factor f;
  unsigned size[IRS_KMAX], stride[IRS_KMAX];
  int ng[IRS_KMAX];
  bool ok = true;
  long sum = 0, groups = 1;
#pragma unroll
  for (int k = 0; k < IRS_KMAX; ++k) {
    const int L = k < K ? lat_sizes[k] : 1, g = k < K ? n_groups[k] : 1;
    ok = ok && L >= 1 && g >= 1 && g <= max_groups;
    size[k] = L >= 1 ? (unsigned)L : 1u;
    ng[k] = g >= 1 ? lesser(g, max_groups) : 1;
  }
  unsigned long long s = 1;
#pragma unroll
  for (int k = IRS_KMAX - 1; k >= 0; --k) {   // a stride that does not fit 32 bits saturates: row numbers are below 2^31, the digit is 0
    stride[k] = (unsigned)s;
    if (k < K) s = lesser(s * size[k], 0xFFFFFFFFull);
  }
  f.size = 1; f.stride = 1; f.voff = 0; f.gbase = 0; f.G = 1;
#pragma unroll
  for (int k = 0; k < IRS_KMAX; ++k) {
    if (k < K) {
      if (k + 1 == j) { f.size = size[k]; f.stride = stride[k]; f.voff = (int)sum; f.gbase = (int)groups; f.G = ng[k]; }
      sum += size[k];
      groups += ng[k];
    }
  }
  f.ok = ok && sum == sum_sizes && groups == total_groups;
  return f;
}
__device__ __forceinline__ bool layout_ok(const int32_t* __restrict__ lat_sizes, const int32_t* __restrict__ n_groups, int K,
                                          long sum_sizes, int total_groups, int max_groups) {
  return load_factor(lat_sizes, n_groups, K, sum_sizes, total_groups, max_groups, 0).ok;
}
// the group of row r within the workgroup's factor, or -1 (j = 0: every row is in group 0)
__device__ __forceinline__ int group_of_row(const Factor& f, const int32_t* __restrict__ group_of_value, int j, unsigned r) {
  if (j == 0) return 0;
  const int g = group_of_value[f.voff + (int)((r / f.stride) % f.size)];
  return (unsigned)g < (unsigned)f.G ? g : -1;
}

// ---- means -------------------------------------------------------------------------------------------------------------------------
// record of one chunk: [total_groups * D] doubles (two words each), then [total_groups] int32 counts
__host__ __device__ __forceinline__ long means_record(int D, int total_groups) { return (2L * D + 1) * total_groups; }

__global__ __launch_bounds__(IRS_T) void k_irs_means_part(const float* __restrict__ table, const int64_t* __restrict__ rows,
                                                          const int32_t* __restrict__ lat_sizes,
                                                          const int32_t* __restrict__ group_of_value,
                                                          const int32_t* __restrict__ n_groups, int D, int K, long S, long sum_sizes,
                                                          int total_groups, int max_groups, long chunk, float* __restrict__ ws) {
  __shared__ float tile[IRS_T][IRS_DC + 1];
  __shared__ int gid[IRS_T];
  const int t = threadIdx.x, j = blockIdx.y;
  const Factor f = load_factor(lat_sizes, n_groups, K, sum_sizes, total_groups, max_groups, j);
  if (!f.ok) return;                                         // (the same in every thread) k_irs_means_finish writes the zeros
  const long c0 = blockIdx.x * chunk, c1 = lesser(S, c0 + chunk);
  const unsigned r0 = rows ? (unsigned)rows[0] : 0u;
  float* rec = ws + blockIdx.x * means_record(D, total_groups);
  float* rec_cnt = rec + 2L * D * total_groups;
  for (int d0 = 0; d0 < D; d0 += IRS_DC) {
    const int dc = lesser(IRS_DC, D - d0), nslot = f.G * dc, ni = (nslot + IRS_T - 1) / IRS_T;   // ni <= IRS_SLOTS
    double acc[IRS_SLOTS], x0[IRS_SLOTS];
    int cnt[IRS_SLOTS], sg[IRS_SLOTS], sd[IRS_SLOTS];
#pragma unroll
    for (int i = 0; i < IRS_SLOTS; ++i) {
      const int slot = t + IRS_T * i;
      acc[i] = 0.;
      cnt[i] = 0;
      sg[i] = slot < nslot ? slot / dc : -2;                 // -2: no slot (gid holds -1 for a row outside every group)
      sd[i] = slot % dc;
      x0[i] = slot < nslot ? (double)table[(long)r0 * D + d0 + sd[i]] : 0.;
    }
    for (long base = c0; base < c1; base += IRS_T) {
      const int nrow = (int)lesser((long)IRS_T, c1 - base);
      if (t < nrow) gid[t] = group_of_row(f, group_of_value, j, rows ? (unsigned)rows[base + t] : (unsigned)(base + t));
      for (int e = t; e < nrow * dc; e += IRS_T) {
        const int rr = e / dc, cc = e % dc;
        const long r = rows ? (long)rows[base + rr] : base + rr;
        tile[rr][cc] = table[r * D + d0 + cc];
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < IRS_SLOTS; ++i) {
        if (i < ni && sg[i] >= 0) {
          for (int rr = 0; rr < nrow; ++rr) {                // in row order
            const bool mine = gid[rr] == sg[i];
            acc[i] += mine ? (double)tile[rr][sd[i]] - x0[i] : 0.;
            cnt[i] += mine ? 1 : 0;
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < IRS_SLOTS; ++i) {
      if (i < ni && sg[i] >= 0) {
        put_f64(rec + 2 * ((long)(f.gbase + sg[i]) * D + d0 + sd[i]), acc[i]);
        if (d0 == 0 && sd[i] == 0) rec_cnt[f.gbase + sg[i]] = __int_as_float(cnt[i]);
      }
    }
  }
}

// one thread per (group, latent): the nb records added in chunk order
__global__ __launch_bounds__(IRS_T) void k_irs_means_finish(const float* __restrict__ table, const int64_t* __restrict__ rows,
                                                            const int32_t* __restrict__ lat_sizes, const int32_t* __restrict__ n_groups,
                                                            int D, int K, long sum_sizes, int total_groups, int max_groups, int nb,
                                                            const float* __restrict__ ws, int32_t* __restrict__ counts,
                                                            float* __restrict__ means) {
  const long e = blockIdx.x * (long)IRS_T + threadIdx.x;
  if (e >= (long)total_groups * D) return;
  const int g = (int)(e / D), d = (int)(e % D);
  if (!layout_ok(lat_sizes, n_groups, K, sum_sizes, total_groups, max_groups)) {
    means[e] = 0.f;
    if (d == 0) counts[g] = 0;
    return;
  }
  const long rec = means_record(D, total_groups);
  double s = 0.;
  long n = 0;
  for (int b = 0; b < nb; ++b) {
    s += get_f64(ws + b * rec + 2 * e);
    n += __float_as_int(ws[b * rec + 2L * D * total_groups + g]);
  }
  const unsigned r0 = rows ? (unsigned)rows[0] : 0u;
  means[e] = n > 0 ? (float)((double)table[(long)r0 * D + d] + s / (double)n) : 0.f;
  if (d == 0) counts[g] = (int)n;
}

// ---- selection ---------------------------------------------------------------------------------------------------------------------
// the words of the workspace, P = total_groups * D (group, latent) pairs: per pair the prefix found so far, the rank that is left
// inside it (-1: skip), the number of deviations <= the result, the smallest deviation above it, the largest; then 256 counters
struct SelectWs {
  unsigned* prefix;
  int* left;
  int* n_le;
  unsigned* next;
  unsigned* largest;
  int* hist;
};
__host__ __device__ __forceinline__ SelectWs select_ws(float* ws, long P) {
  SelectWs w;
  w.prefix = (unsigned*)ws;
  w.left = (int*)ws + P;
  w.n_le = (int*)ws + 2 * P;
  w.next = (unsigned*)ws + 3 * P;
  w.largest = (unsigned*)ws + 4 * P;
  w.hist = (int*)ws + 5 * P;
  return w;
}

__global__ __launch_bounds__(IRS_T) void k_irs_select_init(const int32_t* __restrict__ rank, int D, long P, float* __restrict__ ws) {
  const SelectWs w = select_ws(ws, P);
  const long step = (long)gridDim.x * IRS_T;
  for (long i = blockIdx.x * (long)IRS_T + threadIdx.x; i < P * 256; i += step) {
    w.hist[i] = 0;
    if (i < P) {
      const int k = rank[i / D];
      w.prefix[i] = 0u;
      w.left[i] = k >= 0 ? k : -1;
      w.n_le[i] = 0;
      w.next[i] = IRS_NONE;
      w.largest[i] = 0u;
    }
  }
}

// what a selection workgroup keeps of its slice of groups [g0, g0 + gn) of its factor, for its latent d
struct Slice {
  float centre[IRS_LG];
  unsigned prefix[IRS_LG];
  int live[IRS_LG];
};
__device__ __forceinline__ void load_slice(Slice* sl, const Factor& f, int g0, int gn, int D, int d, const float* __restrict__ centres,
                                           const SelectWs& w) {
  for (int i = threadIdx.x; i < gn; i += IRS_T) {
    const long pair = (long)(f.gbase + g0 + i) * D + d;
    sl->centre[i] = centres[pair];
    sl->prefix[i] = w.prefix[pair];
    sl->live[i] = w.left[pair] >= 0;
  }
}
// the bit pattern of |x - c|: one fp32 subtraction, the sign bit cleared (+0 for x = c)
__device__ __forceinline__ unsigned deviation_bits(float x, float c) { return __float_as_uint(__fsub_rn(x, c)) & 0x7FFFFFFFu; }

// grid (chunks, D, (K + 1) * slices); shift = 24, 16, 8, 0
__global__ __launch_bounds__(IRS_T) void k_irs_select_hist(const float* __restrict__ table, const int64_t* __restrict__ rows,
                                                           const int32_t* __restrict__ lat_sizes,
                                                           const int32_t* __restrict__ group_of_value,
                                                           const int32_t* __restrict__ n_groups, const float* __restrict__ centres, int D,
                                                           int K, long S, long sum_sizes, int total_groups, int max_groups, long chunk,
                                                           int slices, int shift, float* __restrict__ ws) {
  __shared__ int h[IRS_LG * 256];
  __shared__ Slice sl;
  const int t = threadIdx.x, lane = t & 63, d = blockIdx.y, j = blockIdx.z / slices, g0 = (blockIdx.z % slices) * IRS_LG;
  const Factor f = load_factor(lat_sizes, n_groups, K, sum_sizes, total_groups, max_groups, j);
  if (!f.ok || g0 >= f.G) return;                            // (the same in every thread)
  const int gn = lesser(IRS_LG, f.G - g0);
  const SelectWs w = select_ws(ws, (long)total_groups * D);
  load_slice(&sl, f, g0, gn, D, d, centres, w);
  for (int i = t; i < gn * 256; i += IRS_T) h[i] = 0;
  __syncthreads();
  const long c0 = blockIdx.x * chunk, c1 = lesser(S, c0 + chunk);
  for (long base = c0 + (t - lane); base < c1; base += IRS_T) {   // wave-uniform: the ballots below are whole-wave
    const long l = base + lane;
    bool in = l < c1;
    const unsigned r = in ? (rows ? (unsigned)rows[l] : (unsigned)l) : 0u;
    int g = in ? group_of_row(f, group_of_value, j, r) - g0 : -1;
    in = in && g >= 0 && g < gn;
    g = in ? g : 0;
    in = in && sl.live[g];
    const unsigned bits = deviation_bits(table[(long)r * D + d], sl.centre[g]);
    if (shift < 24) in = in && ((bits ^ sl.prefix[g]) >> (shift + 8)) == 0u;   // only the rows inside the group's prefix
    const int key = g * 256 + (int)((bits >> shift) & 255u);
    unsigned long long rest = __ballot(in);
#pragma unroll
    for (int it = 0; it < IRS_AGG; ++it) {                   // a wave's rows mostly share group and leading digit
      if (rest) {
        const int first = __ffsll(rest) - 1;
        const int key0 = __shfl(key, first, 64);
        const unsigned long long m = __ballot(in && key == key0) & rest;
        if (lane == first) atomicAdd(&h[key0], __popcll(m));
        rest &= ~m;
      }
    }
    if ((rest >> lane) & 1ull) atomicAdd(&h[key], 1);
  }
  __syncthreads();
  int* gh = w.hist + ((long)(f.gbase + g0) * D + d) * 256;
  for (int i = t; i < gn * 256; i += IRS_T) {
    const int cnt = h[i];
    if (cnt) atomicAdd(&gh[(long)(i >> 8) * D * 256 + (i & 255)], cnt);
  }
}

// one wave per (group, latent) pair: the bin that holds the rank.  Lane l owns bins 4 l .. 4 l + 3.
__global__ __launch_bounds__(IRS_T) void k_irs_select_walk(const int32_t* __restrict__ rank, int D, long P, int pass, int shift,
                                                           float* __restrict__ ws) {
  const SelectWs w = select_ws(ws, P);
  const int lane = threadIdx.x & 63;
  const long pair = blockIdx.x * (long)(IRS_T / 64) + (threadIdx.x >> 6);
  if (pair >= P) return;                                     // (the same in every lane of the wave)
  int* hp = w.hist + pair * 256 + lane * 4;
  int c[4], own = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    c[i] = hp[i];
    hp[i] = 0;                                               // for the next pass
    own += c[i];
  }
  int incl = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  const int total = __shfl(incl, 63, 64);
  int k = w.left[pair];
  if (pass == 0 && k >= total) {                             // a rank outside [0, n_g): the group is skipped from here on
    if (lane == 0) w.left[pair] = -1;
    return;
  }
  if (k < 0) return;
  int below = incl - own;                                    // deviations in the bins of the lanes before this one
  if (below <= k && k < incl) {                              // exactly one lane
    int digit = lane * 4 + 3, in_bin = c[3];
    bool found = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (!found) {
        if (k < below + c[i]) {
          found = true;
          digit = lane * 4 + i;
          in_bin = c[i];
        } else {
          below += c[i];
        }
      }
    }
    w.prefix[pair] |= (unsigned)digit << shift;
    w.left[pair] = k - below;
    if (pass == DVAE_IRS_SELECT_PASSES - 1) w.n_le[pair] = rank[pair / D] - (k - below) + in_bin;
  }
}

// grid as k_irs_select_hist: the largest deviation and the smallest one above the selected value, per group
__global__ __launch_bounds__(IRS_T) void k_irs_select_next(const float* __restrict__ table, const int64_t* __restrict__ rows,
                                                           const int32_t* __restrict__ lat_sizes,
                                                           const int32_t* __restrict__ group_of_value,
                                                           const int32_t* __restrict__ n_groups, const float* __restrict__ centres, int D,
                                                           int K, long S, long sum_sizes, int total_groups, int max_groups, long chunk,
                                                           int slices, float* __restrict__ ws) {
  __shared__ unsigned largest[IRS_LG], next[IRS_LG];
  __shared__ Slice sl;
  const int t = threadIdx.x, d = blockIdx.y, j = blockIdx.z / slices, g0 = (blockIdx.z % slices) * IRS_LG;
  const Factor f = load_factor(lat_sizes, n_groups, K, sum_sizes, total_groups, max_groups, j);
  if (!f.ok || g0 >= f.G) return;
  const int gn = lesser(IRS_LG, f.G - g0);
  const SelectWs w = select_ws(ws, (long)total_groups * D);
  load_slice(&sl, f, g0, gn, D, d, centres, w);
  if (t < gn) { largest[t] = 0u; next[t] = IRS_NONE; }
  __syncthreads();
  const long c0 = blockIdx.x * chunk, c1 = lesser(S, c0 + chunk);
  for (long l = c0 + t; l < c1; l += IRS_T) {
    const unsigned r = rows ? (unsigned)rows[l] : (unsigned)l;
    const int g = group_of_row(f, group_of_value, j, r) - g0;
    if (g < 0 || g >= gn || !sl.live[g]) continue;
    const unsigned bits = deviation_bits(table[(long)r * D + d], sl.centre[g]);
    // a plain look first: after a few rows almost none improves on what is there, and the atomic decides in any case
    if (bits > *(volatile unsigned*)&largest[g]) atomicMax(&largest[g], bits);
    if (bits > sl.prefix[g] && bits < *(volatile unsigned*)&next[g]) atomicMin(&next[g], bits);
  }
  __syncthreads();
  if (t < gn && sl.live[t]) {
    const long pair = (long)(f.gbase + g0 + t) * D + d;
    if (largest[t] != 0u) atomicMax(&w.largest[pair], largest[t]);
    if (next[t] != IRS_NONE) atomicMin(&w.next[pair], next[t]);
  }
}

__global__ __launch_bounds__(IRS_T) void k_irs_select_finish(const int32_t* __restrict__ lat_sizes, const int32_t* __restrict__ n_groups,
                                                             const int32_t* __restrict__ rank, int D, int K, long sum_sizes,
                                                             int total_groups, int max_groups, float* __restrict__ ws,
                                                             float* __restrict__ stat_lo, float* __restrict__ stat_hi,
                                                             float* __restrict__ dev_max) {
  const long P = (long)total_groups * D, pair = blockIdx.x * (long)IRS_T + threadIdx.x;
  if (pair >= P) return;
  const SelectWs w = select_ws(ws, P);
  unsigned lo = 0u, hi = 0u, mx = 0u;
  if (layout_ok(lat_sizes, n_groups, K, sum_sizes, total_groups, max_groups) && w.left[pair] >= 0) {
    lo = w.prefix[pair];
    const unsigned nx = w.next[pair];
    // more than rank + 1 deviations are <= lo: the next one in order is lo again; else the smallest larger one (none: rank = n_g - 1)
    hi = (w.n_le[pair] > rank[pair / D] + 1 || nx == IRS_NONE) ? lo : nx;
    mx = w.largest[pair];
  }
  stat_lo[pair] = __uint_as_float(lo);
  stat_hi[pair] = __uint_as_float(hi);
  dev_max[pair] = __uint_as_float(mx);
}

bool sizes_ok(long N, int D, int K, long S, int total_groups) {
  return N > 0 && N <= 2147483647L && D > 0 && D <= 65535 && K > 0 && K <= DVAE_IRS_MAX_FACTORS && S > 0 && S <= 2147483647L &&
         total_groups >= 1 + K && total_groups <= 1 + K * DVAE_IRS_MAX_GROUPS && (long)total_groups * D <= DVAE_IRS_MAX_PAIRS;
}

}  // namespace
}  // namespace dvae

using namespace dvae;

extern "C" {

int dvae_irs_version(void) { return DVAE_IRS_VERSION; }
const char* dvae_irs_last_error(void) { return last_error(); }

size_t dvae_irs_group_means_ws_floats(long N, int D, int K, long S, int total_groups) {
  if (S <= 0) S = N;
  if (!sizes_ok(N, D, K, S, total_groups)) return 0;
  long chunk;
  const int nb = chunks_of(S, DVAE_IRS_MEANS_BLOCK_ROWS, DVAE_IRS_MAX_BLOCKS, &chunk);
  return (size_t)(nb * means_record(D, total_groups));
}

size_t dvae_irs_group_order_stats_ws_floats(long N, int D, int K, long S, int total_groups) {
  if (S <= 0) S = N;
  if (!sizes_ok(N, D, K, S, total_groups)) return 0;
  return (size_t)((long)total_groups * D * (256 + 5));
}

int dvae_irs_group_means(const float* table, const int64_t* rows, const int32_t* lat_sizes, const int32_t* group_of_value,
                         const int32_t* n_groups, long N, int D, int K, long S, long sum_sizes, int total_groups, int max_groups,
                         float* ws, int32_t* counts, float* means, void* stream) {
  if (!rows) S = N;
  DVAE_CHECK_ARG(table && lat_sizes && group_of_value && n_groups && ws && counts && means);
  DVAE_CHECK_ARG(K <= DVAE_IRS_MAX_FACTORS);
  DVAE_CHECK_ARG(max_groups <= DVAE_IRS_MAX_GROUPS);
  DVAE_CHECK_ARG(sizes_ok(N, D, K, S, total_groups));
  DVAE_CHECK_ARG(max_groups >= 1 && sum_sizes >= K && sum_sizes <= 2147483647L && total_groups <= 1 + (long)K * max_groups);
  hipStream_t st = (hipStream_t)stream;
  long chunk;
  const int nb = chunks_of(S, DVAE_IRS_MEANS_BLOCK_ROWS, DVAE_IRS_MAX_BLOCKS, &chunk);
  hipLaunchKernelGGL(k_irs_means_part, dim3(nb, K + 1), dim3(IRS_T), 0, st, table, rows, lat_sizes, group_of_value, n_groups, D, K, S,
                     sum_sizes, total_groups, max_groups, chunk, ws);
  DVAE_CHECK_LAUNCH();
  const long P = (long)total_groups * D;
  hipLaunchKernelGGL(k_irs_means_finish, dim3((unsigned)((P + IRS_T - 1) / IRS_T)), dim3(IRS_T), 0, st, table, rows, lat_sizes, n_groups,
                     D, K, sum_sizes, total_groups, max_groups, nb, ws, counts, means);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int dvae_irs_group_order_stats(const float* table, const int64_t* rows, const int32_t* lat_sizes, const int32_t* group_of_value,
                               const int32_t* n_groups, const float* centres, const int32_t* rank, long N, int D, int K, long S,
                               long sum_sizes, int total_groups, int max_groups, float* ws, float* stat_lo, float* stat_hi,
                               float* dev_max, void* stream) {
  if (!rows) S = N;
  DVAE_CHECK_ARG(table && lat_sizes && group_of_value && n_groups && centres && rank && ws && stat_lo && stat_hi && dev_max);
  DVAE_CHECK_ARG(K <= DVAE_IRS_MAX_FACTORS);
  DVAE_CHECK_ARG(max_groups <= DVAE_IRS_MAX_GROUPS);
  DVAE_CHECK_ARG(sizes_ok(N, D, K, S, total_groups));
  DVAE_CHECK_ARG(max_groups >= 1 && sum_sizes >= K && sum_sizes <= 2147483647L && total_groups <= 1 + (long)K * max_groups);
  hipStream_t st = (hipStream_t)stream;
  const long P = (long)total_groups * D;
  long chunk;
  const int nb = chunks_of(S, DVAE_IRS_SELECT_BLOCK_ROWS, DVAE_IRS_MAX_BLOCKS, &chunk);
  const int slices = (max_groups + IRS_LG - 1) / IRS_LG;
  const dim3 grid(nb, D, (K + 1) * slices);
  hipLaunchKernelGGL(k_irs_select_init, dim3((unsigned)lesser((P * 256 + IRS_T - 1) / IRS_T, 4096L)), dim3(IRS_T), 0, st, rank, D, P, ws);
  DVAE_CHECK_LAUNCH();
  for (int pass = 0; pass < DVAE_IRS_SELECT_PASSES; ++pass) {
    const int shift = 24 - 8 * pass;
    hipLaunchKernelGGL(k_irs_select_hist, grid, dim3(IRS_T), 0, st, table, rows, lat_sizes, group_of_value, n_groups, centres, D, K, S,
                       sum_sizes, total_groups, max_groups, chunk, slices, shift, ws);
    DVAE_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_irs_select_walk, dim3((unsigned)((P + IRS_T / 64 - 1) / (IRS_T / 64))), dim3(IRS_T), 0, st, rank, D, P, pass, shift,
                       ws);
    DVAE_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_irs_select_next, grid, dim3(IRS_T), 0, st, table, rows, lat_sizes, group_of_value, n_groups, centres, D, K, S,
                     sum_sizes, total_groups, max_groups, chunk, slices, ws);
  DVAE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_irs_select_finish, dim3((unsigned)((P + IRS_T - 1) / IRS_T)), dim3(IRS_T), 0, st, lat_sizes, n_groups, rank, D, K,
                     sum_sizes, total_groups, max_groups, ws, stat_lo, stat_hi, dev_max);
  DVAE_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
