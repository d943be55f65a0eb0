// libdvae_unsup_hip.so (include/dvae_unsup_hip.h): the two latent-with-latent statistics of the [N, D] table of posterior means
// behind the label-free scores of disentanglement_lib's unsupervised_metrics -- the full D x D covariance (Gaussian total
// correlation, Gaussian Wasserstein correlation) and the D (D - 1) / 2 joint histograms of every pair of discretised latents
// (mean pairwise mutual information) -- over S selected rows.  No factor of variation appears anywhere.
//
// Moments.  A workgroup owns one chunk of rows and walks it in blocks of UNSUP_STAGE_ROWS rows staged through LDS: the D floats
// of a row are consecutive in memory, consecutive threads load consecutive floats, and column D of the staged line holds 1.  The
// D (D + 3) / 2 sums -- (d, e) with d <= e <= D; e = D is the plain sum of column d -- are dealt to the threads round robin, up to
// DVAE_UNSUP_MOMENTS_THREAD_SUMS each; a thread walks the staged rows in order and adds (x_d - x0_d)(x_e - x0_e) in fp64
// registers, each float converted BEFORE the subtraction (x0 = the first selected row; x0_D = 0).  The owner of (d, D) keeps
// min and max of column d as well.  One record of partial sums per chunk; k_unsup_moments_finish gives a wave to every sum: lane
// l adds chunks l, l + 64, ... in order, then the xor butterfly -- a fixed order, no atomics, the same bits every run -- and
// writes mean, or cov[d, e] and cov[e, d] from the one value.
//
// Histograms.  Grid = (chunks of rows, tiles of consecutive pairs); a tile is as many pairs as DVAE_UNSUP_HIST_LDS_INTS counters
// hold.  Per block of 256 rows the workgroup first bins every (row, latent the tile touches) once -- consecutive threads take the
// consecutive latents of a row, so the loads coalesce; the bin is a count of edges <= x against edges kept in LDS -- and stages
// the bins as bytes, a row's bytes at an odd stride of words.  Then a thread per row adds one counter per pair of the tile.
// Trained VAEs have collapsed dimensions: every row lands in ONE bin of such a latent, so for a pair of two of them all 64 lanes
// of a wave would queue on one LDS address.  A wave whose valid rows share the cell (one vote against lane 0's) adds their
// number once instead; every other pair takes plain LDS integer atomics, which a live latent spreads over its bins.  The
// workgroup adds its non-zero counters to `counts` at its end (integer adds: any order gives the same counts);
// k_unsup_zero clears `counts` first.
#include "../../include/dvae_unsup_hip.h"
#include "common.h"
#include "last_error.h"
#include "table_stats.h"

namespace dvae {

namespace {

#define UNSUP_T 256
#define UNSUP_DMAX DVAE_UNSUP_MAX_D
#define UNSUP_STAGE_ROWS 64                                   // rows of one staged block of the moments pass
#define UNSUP_SUMS DVAE_UNSUP_MOMENTS_THREAD_SUMS
#define UNSUP_EDGE_FLOATS 1024                                // edges of the latents of one tile (host-checked; 704 suffice)
#define UNSUP_BIN_STRIDE_MAX (UNSUP_DMAX + 4)                 // bytes of one row's staged bins, at most

static_assert(UNSUP_SUMS * UNSUP_T >= UNSUP_DMAX * (UNSUP_DMAX + 3) / 2, "every sum needs an owner");
static_assert(DVAE_UNSUP_MAX_BINS <= 256, "a bin is staged as one byte");
static_assert(DVAE_UNSUP_HIST_LDS_INTS >= DVAE_UNSUP_MAX_BINS * DVAE_UNSUP_MAX_BINS, "one pair of the most bins fits a tile");

// ---- moments --------------------------------------------------------------------------------------------------------------------
// sum i <-> (a, b), a <= b <= D, in lexicographic order: line a holds D + 1 - a of them
__host__ __device__ __forceinline__ int n_sums(int D) { return D * (D + 3) / 2; }
__device__ __forceinline__ int sum_index(int a, int b, int D) { return a * (D + 1) - a * (a - 1) / 2 + (b - a); }
__device__ __forceinline__ void sum_pair(int i, int D, int* a, int* b) {
  int d = 0;
  while (i >= D + 1 - d) { i -= D + 1 - d; ++d; }
  *a = d;
  *b = d + i;
}
// record of one chunk, in fp32 words: [n_sums] doubles, then min [D] and max [D] as floats
__host__ __device__ __forceinline__ long moments_record(int D) { return 2L * n_sums(D) + 2L * D; }

__global__ __launch_bounds__(UNSUP_T) void k_unsup_moments_part(const float* __restrict__ table, const int64_t* __restrict__ rows,
                                                                int D, long S, long chunk, float* __restrict__ ws) {
  __shared__ float sx[UNSUP_STAGE_ROWS * (UNSUP_DMAX + 1)];
  const int t = threadIdx.x, W = D + 1, ns = n_sums(D);
  const long r0 = rows ? (long)rows[0] : 0L;
  const long c0 = blockIdx.x * chunk, c1 = lesser(S, c0 + chunk);
  int ia[UNSUP_SUMS], ib[UNSUP_SUMS];                        // the staged columns of this thread's sums (sum j: number j * 256 + t)
  double x0a[UNSUP_SUMS], x0b[UNSUP_SUMS], acc[UNSUP_SUMS];
#pragma unroll
  for (int j = 0; j < UNSUP_SUMS; ++j) {
    ia[j] = ib[j] = 0;
    x0a[j] = x0b[j] = acc[j] = 0.;
    if (j * UNSUP_T + t < ns) {
      sum_pair(j * UNSUP_T + t, D, &ia[j], &ib[j]);
      x0a[j] = (double)table[r0 * D + ia[j]];
      x0b[j] = ib[j] < D ? (double)table[r0 * D + ib[j]] : 0.;   // column D is 1: (1 - 0) leaves the plain sum of column a
    }
  }
  float mn[UNSUP_SUMS], mx[UNSUP_SUMS];                      // of column ia[j], kept where ib[j] == D
#pragma unroll
  for (int j = 0; j < UNSUP_SUMS; ++j) { mn[j] = INFINITY; mx[j] = -INFINITY; }
  for (long base = c0; base < c1; base += UNSUP_STAGE_ROWS) {
    const int nrows = (int)lesser((long)UNSUP_STAGE_ROWS, c1 - base);
    __syncthreads();                                         // the previous block's reads are done
    for (int i = t; i < nrows * D; i += UNSUP_T) {
      const int r = i / D, c = i - r * D;
      const long row = rows ? (long)rows[base + r] : base + r;
      sx[r * W + c] = table[row * D + c];
    }
    if (t < nrows) sx[t * W + D] = 1.f;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < UNSUP_SUMS; ++j) {
      if (j * UNSUP_T + t < ns) {
        const float* pa = sx + ia[j];
        const float* pb = sx + ib[j];
        double s = acc[j];
#pragma unroll 4
        for (int r = 0; r < nrows; ++r) s = fma((double)pa[r * W] - x0a[j], (double)pb[r * W] - x0b[j], s);
        acc[j] = s;
        if (ib[j] == D) {
#pragma unroll 4
          for (int r = 0; r < nrows; ++r) {
            mn[j] = fminf(mn[j], pa[r * W]);
            mx[j] = fmaxf(mx[j], pa[r * W]);
          }
        }
      }
    }
  }
  float* rec = ws + blockIdx.x * moments_record(D);
#pragma unroll
  for (int j = 0; j < UNSUP_SUMS; ++j) {
    if (j * UNSUP_T + t < ns) {
      put_f64(rec + 2 * (j * UNSUP_T + t), acc[j]);
      if (ib[j] == D) {
        rec[2 * ns + ia[j]] = mn[j];
        rec[2 * ns + D + ia[j]] = mx[j];
      }
    }
  }
}

// fixed-order sum of word pair `i` of every chunk's record by one wave: lane l takes chunks l, l + 64, ... in order
__device__ __forceinline__ double wave_sum_chunks(const float* __restrict__ ws, long rec, int nb, int i, int lane) {
  double v = 0.;
  for (int b = lane; b < nb; b += 64) v += get_f64(ws + b * rec + 2 * i);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(UNSUP_T) void k_unsup_moments_finish(const float* __restrict__ table, const int64_t* __restrict__ rows,
                                                                  int D, long S, int nb, const float* __restrict__ ws,
                                                                  float* __restrict__ col_min, float* __restrict__ col_max,
                                                                  double* __restrict__ col_mean, double* __restrict__ cov) {
  const int lane = threadIdx.x & 63, ns = n_sums(D);
  const int i = blockIdx.x * (UNSUP_T / 64) + (threadIdx.x >> 6);   // the same in every lane of a wave
  if (i >= ns) return;
  const long rec = moments_record(D);
  int a, b;
  sum_pair(i, D, &a, &b);
  const double n = (double)S;
  const double s1a = wave_sum_chunks(ws, rec, nb, sum_index(a, D, D), lane);
  if (b == D) {
    float mn = INFINITY, mx = -INFINITY;
    for (int c = lane; c < nb; c += 64) {
      mn = fminf(mn, ws[c * rec + 2 * ns + a]);
      mx = fmaxf(mx, ws[c * rec + 2 * ns + D + a]);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      mn = fminf(mn, __shfl_xor(mn, o, 64));
      mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if (lane == 0) {
      const long r0 = rows ? (long)rows[0] : 0L;
      col_min[a] = mn;
      col_max[a] = mx;
      col_mean[a] = (double)table[r0 * D + a] + s1a / n;
    }
    return;
  }
  const double s1b = wave_sum_chunks(ws, rec, nb, sum_index(b, D, D), lane);
  const double s2 = wave_sum_chunks(ws, rec, nb, i, lane);
  if (lane == 0) {
    const double c = S > 1 ? (s2 - s1a * s1b / n) / (double)(S - 1) : 0.;
    cov[(long)a * D + b] = c;
    cov[(long)b * D + a] = c;
  }
}

// ---- histograms -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(UNSUP_T) void k_unsup_zero(int32_t* __restrict__ p, long n) {
  zero_i32<UNSUP_T>(p, n);
}

// pair p <-> (d, e), d < e < D, in lexicographic order: line d holds D - 1 - d of them
__device__ __forceinline__ void pair_of(int p, int D, int* d, int* e) {
  int a = 0;
  while (p >= D - 1 - a) { p -= D - 1 - a; ++a; }
  *d = a;
  *e = a + 1 + p;
}
__device__ __forceinline__ void next_pair(int D, int* d, int* e) {
  if (++*e == D) { ++*d; *e = *d + 1; }
}
// bytes between the staged bins of two rows: a multiple of 4 that is an odd number of words, so 64 rows meet 64 banks
__host__ __device__ __forceinline__ int bin_stride(int slots) {
  const int words = (slots + 3) / 4;
  return 4 * (words | 1);
}

__global__ __launch_bounds__(UNSUP_T) void k_unsup_pair_hist(const float* __restrict__ table, const int64_t* __restrict__ rows,
                                                             const float* __restrict__ edges, int D, long S, int n_bins, long chunk,
                                                             int P, int tile_pairs, int32_t* __restrict__ counts) {
  __shared__ int h[DVAE_UNSUP_HIST_LDS_INTS];
  __shared__ float edge[UNSUP_EDGE_FLOATS];                  // [slot][n_bins]
  __shared__ unsigned char binb[UNSUP_T * UNSUP_BIN_STRIDE_MAX];   // [row of the block][slot]
  __shared__ unsigned char slot_of[UNSUP_DMAX], lat_of[UNSUP_DMAX];
  __shared__ unsigned long long touched_mask;
  const int t = threadIdx.x, lane = t & 63, nb2 = n_bins * n_bins;
  const int p0 = blockIdx.y * tile_pairs, np = lesser(tile_pairs, P - p0);
  int d0, e0;
  pair_of(p0, D, &d0, &e0);
  if (t == 0) {                                              // the latents of this tile's pairs
    unsigned long long m = 0;
    int d = d0, e = e0;
    for (int q = 0; q < np; ++q) {
      m |= (1ull << d) | (1ull << e);
      next_pair(D, &d, &e);
    }
    touched_mask = m;
  }
  for (int i = t; i < np * nb2; i += UNSUP_T) h[i] = 0;
  __syncthreads();
  const unsigned long long mask = touched_mask;
  const int L = __popcll(mask), Ls = bin_stride(L);          // slots: the touched latents in ascending order; L >= 2
  if (t < D && ((mask >> t) & 1ull)) {
    const int s = __popcll(mask & ((1ull << t) - 1ull));
    slot_of[t] = (unsigned char)s;
    lat_of[s] = (unsigned char)t;
  }
  __syncthreads();
  for (int i = t; i < L * n_bins; i += UNSUP_T) edge[i] = edges[(long)lat_of[i / n_bins] * n_bins + i % n_bins];
  const long c0 = blockIdx.x * chunk, c1 = lesser(S, c0 + chunk);
  const int step_rows = UNSUP_T / L, step_slots = UNSUP_T % L;
  for (long base = c0; base < c1; base += UNSUP_T) {
    const int nrows = (int)lesser((long)UNSUP_T, c1 - base);
    __syncthreads();                                         // edge is written; the previous block's bins are read
    // element t, t + 256, ... of the [nrows, L] block: bin it once, stage the byte
    for (int r = t / L, s = t % L; r < nrows;) {
      const long row = rows ? (long)rows[base + r] : base + r;
      const float x = table[row * D + lat_of[s]];
      const float* ed = edge + s * n_bins;
      // (the count of edges stays in the kernel: as a helper shared with k_info_joint_hist it changed both kernels' machine code)
      int below = 0;
      for (int j = 0; j < n_bins; ++j) below += ed[j] <= x ? 1 : 0;
      binb[r * Ls + s] = (unsigned char)min(max(below - 1, 0), n_bins - 1);
      r += step_rows;
      s += step_slots;
      if (s >= L) { s -= L; ++r; }
    }
    __syncthreads();
    if (t - lane < nrows) {                                  // wave-uniform: the vote and the ballot below are whole-wave
      const bool valid = t < nrows;                          // (lane 0 always is)
      const int n_valid = __popcll(__ballot(valid));        // taken by the whole wave, not inside lane 0's branch
      const unsigned char* mine = binb + t * Ls;
      int d = d0, e = e0, ba = mine[slot_of[d0]];
      for (int q = 0; q < np; ++q) {
        const int cell = q * nb2 + ba * n_bins + mine[slot_of[e]];
        const int first = __builtin_amdgcn_readfirstlane(cell);
        if (__all(!valid || cell == first)) {                // (two collapsed latents) one add for the wave
          if (lane == 0) atomicAdd(&h[first], n_valid);
        } else if (valid) {
          atomicAdd(&h[cell], 1);
        }
        next_pair(D, &d, &e);
        if (e == d + 1 && q + 1 < np) ba = mine[slot_of[d]];
      }
    }
  }
  __syncthreads();
  int32_t* gcnt = counts + (long)p0 * nb2;
  for (int i = t; i < np * nb2; i += UNSUP_T) {
    const int cnt = h[i];
    if (cnt) atomicAdd(&gcnt[i], cnt);
  }
}

bool sizes_ok(long N, int D, long S) {
  return N > 0 && N <= 2147483647L && D > 0 && D <= DVAE_UNSUP_MAX_D && S > 0 && S <= 2147483647L;
}

}  // namespace
}  // namespace dvae

using namespace dvae;

extern "C" {

int dvae_unsup_version(void) { return DVAE_UNSUP_VERSION; }
const char* dvae_unsup_last_error(void) { return last_error(); }

size_t dvae_unsup_moments_ws_floats(long N, int D, long S) {
  if (S <= 0) S = N;
  if (!sizes_ok(N, D, S)) return 0;
  long chunk;
  const int nb = chunks_of(S, DVAE_UNSUP_MOMENTS_BLOCK_ROWS, DVAE_UNSUP_MAX_BLOCKS, &chunk);
  return (size_t)(nb * moments_record(D));                   // one record per chunk
}

size_t dvae_unsup_pair_hist_ws_floats(long N, int D, long S, int n_bins) {
  (void)N; (void)D; (void)S; (void)n_bins;
  return 0;                                                    // the counters are integers: added where they lie
}

int dvae_unsup_moments(const float* table, const int64_t* rows, long N, int D, long S, float* ws, float* col_min, float* col_max,
                       double* col_mean, double* cov, void* stream) {
  if (!rows) S = N;
  DVAE_CHECK_ARG(table && ws && col_min && col_max && col_mean && cov);
  DVAE_CHECK_ARG(D <= DVAE_UNSUP_MAX_D);
  DVAE_CHECK_ARG(sizes_ok(N, D, S));
  hipStream_t st = (hipStream_t)stream;
  long chunk;
  const int nb = chunks_of(S, DVAE_UNSUP_MOMENTS_BLOCK_ROWS, DVAE_UNSUP_MAX_BLOCKS, &chunk);
  hipLaunchKernelGGL(k_unsup_moments_part, dim3(nb), dim3(UNSUP_T), 0, st, table, rows, D, S, chunk, ws);
  DVAE_CHECK_LAUNCH();
  const int waves = UNSUP_T / 64;
  hipLaunchKernelGGL(k_unsup_moments_finish, dim3((n_sums(D) + waves - 1) / waves), dim3(UNSUP_T), 0, st, table, rows, D, S, nb, ws,
                     col_min, col_max, col_mean, cov);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int dvae_unsup_pair_hist(const float* table, const int64_t* rows, const float* edges, long N, int D, long S, int n_bins, float* ws,
                         int32_t* counts, void* stream) {
  (void)ws;
  if (!rows) S = N;
  DVAE_CHECK_ARG(table && edges && counts);
  DVAE_CHECK_ARG(D <= DVAE_UNSUP_MAX_D);
  DVAE_CHECK_ARG(n_bins >= 1 && n_bins <= DVAE_UNSUP_MAX_BINS);
  DVAE_CHECK_ARG(sizes_ok(N, D, S));
  DVAE_CHECK_ARG(D >= 2);                                      // one latent has no pair
  hipStream_t st = (hipStream_t)stream;
  const int P = D * (D - 1) / 2, nb2 = n_bins * n_bins;
  const int tile_pairs = lesser(P, DVAE_UNSUP_HIST_LDS_INTS / nb2 > 1 ? DVAE_UNSUP_HIST_LDS_INTS / nb2 : 1);
  // a tile of q pairs touches 2 q latents at most: their edges and a row's bins must fit what the kernel stages
  DVAE_CHECK_ARG(lesser(D, 2 * tile_pairs) * n_bins <= UNSUP_EDGE_FLOATS && bin_stride(lesser(D, 2 * tile_pairs)) <= UNSUP_BIN_STRIDE_MAX);
  const long all = (long)P * nb2;
  hipLaunchKernelGGL(k_unsup_zero, dim3((unsigned)lesser((all + UNSUP_T - 1) / UNSUP_T, 1024L)), dim3(UNSUP_T), 0, st, counts, all);
  DVAE_CHECK_LAUNCH();
  long chunk;
  const int nb = chunks_of(S, DVAE_UNSUP_HIST_BLOCK_ROWS, DVAE_UNSUP_MAX_BLOCKS, &chunk);
  hipLaunchKernelGGL(k_unsup_pair_hist, dim3(nb, (P + tile_pairs - 1) / tile_pairs), dim3(UNSUP_T), 0, st, table, rows, edges, D, S,
                     n_bins, chunk, P, tile_pairs, counts);
  DVAE_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
