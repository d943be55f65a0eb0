// libdvae_knn_hip.so (include/dvae_knn_hip.h): the binning-free mutual information between a continuous latent and a discrete
// factor -- the k-nearest-neighbour estimator of Ross 2014 (scikit-learn's _compute_mi_cd) for every (latent, factor) pair.  In one
// dimension it needs no tree: a sort, a partition by label, a bounded neighbour walk and two binary searches per row.
//
// k_knn_sort.  One workgroup per latent column.  A value becomes the 32-bit key of latent_ranks.hip (unsigned order = numeric
// order, -0 folded into +0; bit operations only, so denormals stay what they are) and (key, selection index) one 64-bit word; the
// column, padded to a power of two with all-ones words, is sorted in LDS by a bitonic network -- compare-exchanges of 64-bit
// integers, in place, so 8 bytes per row where a radix sort's ping-pong buffers take 16 and do not fit 16 384 rows.  The words are
// distinct, so the result does not depend on the network: equal values lie in the order of their selection indices.
// k_knn_mi.  One workgroup per (latent d, factor k); everything below happens in its LDS.
//   load     the sorted values and selection indices of column d; the label of a row is (row / stride_k) % size_k of its ROW
//            NUMBER; the classes are counted by integer adds.
//   split    ONE forward pass over the sorted list in tiles of the workgroup's threads.  A row is kept when its class has two rows
//            or more.  Its place q in the compacted list is the number of kept rows before it (a ballot, a population count below
//            the lane, the waves before its own); its place j in the list of its class is the class's start plus the number of
//            its class before it (the eight ballots of latent_ranks.hip's scatter).  Both are stable, so the compacted list and
//            every class list stay sorted.  The compaction is in place (q <= position, and a tile is read before a barrier and
//            written after it); the class lists hold q, not the value: 2 bytes per row.
//   walk     row j of a class list steps outwards k_i = min(kn, c_i - 1) times to the nearer of its two next neighbours in the
//            list; the last step's distance is r_i.  Differences are fp64 differences of the converted floats.
//   search   m_i: the first place at or before q and the last at or after q whose distance is inside r_i (strictly below it, or
//            equal to 0 where r_i is 0), by bisection with a fixed number of steps.
//   sum      thread t adds psi[k_i], psi[c_i], psi[m_i] of rows t, t + 512, ... in that order; a fixed shuffle tree per wave, the
//            waves in their order by thread 0.
#include <math.h>

#include "../../include/dvae_knn_hip.h"
#include "common.h"
#include "last_error.h"

namespace dvae {

namespace {

#define KNN_ST DVAE_KNN_SORT_THREADS
#define KNN_T DVAE_KNN_MI_THREADS
#define KNN_WAVES (KNN_T / 64)
#define KNN_C DVAE_KNN_MAX_CLASSES
#define KNN_BISECT 15                                            // steps of a bisection over at most 2^15 places

static_assert(KNN_ST % 64 == 0 && KNN_ST <= 1024 && KNN_T % 64 == 0 && KNN_T <= 1024 && KNN_T >= KNN_C, "whole waves; thread v owns class v");
static_assert(DVAE_KNN_MAX_ROWS >= 10240, "DCI's row count runs from LDS");
static_assert(DVAE_KNN_MAX_ROWS <= 65536 && DVAE_KNN_MAX_ROWS <= (1 << KNN_BISECT), "places are uint16; the bisection's steps");
static_assert((DVAE_KNN_MAX_ROWS & (DVAE_KNN_MAX_ROWS - 1)) == 0, "the padded column of the sort is DVAE_KNN_MAX_ROWS at most");
static_assert(DVAE_KNN_MAX_CLASSES <= 256, "a label is one byte and one 8-bit digit");
static_assert((long)DVAE_KNN_SORT_ROW_BYTES * DVAE_KNN_MAX_ROWS <= 160L * 1024, "the LDS of one CU");
static_assert((long)DVAE_KNN_MI_ROW_BYTES * DVAE_KNN_MAX_ROWS + DVAE_KNN_MI_FIXED_BYTES <= 160L * 1024, "the LDS of one CU");

struct Factors {
  int size[DVAE_KNN_MAX_FACTORS];                                // values of factor k (1 beyond K)
  int offset[DVAE_KNN_MAX_FACTORS];                              // the sizes before it, summed
  long stride[DVAE_KNN_MAX_FACTORS];                             // row-major: prod(size[k + 1 ..])
};

struct MiTables {                                                // the fixed part of k_knn_mi's LDS
  int cnt[KNN_C];                                                // rows of class v among the S selected
  int cstart[KNN_C];                                             // where the list of class v starts among the class lists
  int cpos[KNN_C];                                               // where its next row goes (the split)
  int wave_cnt[KNN_WAVES * KNN_C];                               // rows of class v in wave w of the current tile
  int wave_keep[KNN_WAVES];                                      // kept rows in wave w of the current tile
  double red[KNN_WAVES * 3];
};
static_assert(sizeof(MiTables) <= DVAE_KNN_MI_FIXED_BYTES, "the header's LDS plan");

// unsigned order of the key = numeric order of the float; -0 and +0 give one key (latent_ranks.hip)
__device__ __forceinline__ uint32_t key_of(float x) {
  uint32_t u = __float_as_uint(x);
  if ((u << 1) == 0u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t key) {
  return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// the lanes of this wave that are valid and hold the same 8-bit digit as the caller (0 for an invalid lane); whole-wave
__device__ __forceinline__ unsigned long long same_digit(uint32_t digit, bool valid) {
  unsigned long long m = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (digit >> b) & 1u;
    const unsigned long long v = __ballot(bit);
    m &= bit ? v : ~v;
  }
  return valid ? m : 0ull;
}

__global__ __launch_bounds__(KNN_ST) void k_knn_sort(const float* __restrict__ table, const int64_t* __restrict__ rows, int D, int S,
                                                     int P2, float* __restrict__ vals, int32_t* __restrict__ idx) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long pairs[];   // [P2]
  const int t = threadIdx.x, d = blockIdx.x;
  for (int p = t; p < P2; p += KNN_ST) {
    unsigned long long v = ~0ull;                                // the padding: above every pair
    if (p < S) {
      const long row = rows ? (long)rows[p] : (long)p;
      v = ((unsigned long long)key_of(table[row * D + d]) << 32) | (unsigned long long)(uint32_t)p;
    }
    pairs[p] = v;
  }
  __syncthreads();
  for (int k = 2; k <= P2; k <<= 1) {                            // the bitonic network: log2(P2) (log2(P2) + 1) / 2 steps
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < (P2 >> 1); i += KNN_ST) {
        const int a = ((i & ~(j - 1)) << 1) | (i & (j - 1)), b = a | j;        // a < b < P2, bit j of a clear
        const bool up = (a & k) == 0;
        const unsigned long long va = pairs[a], vb = pairs[b];
        if ((va > vb) == up) {
          pairs[a] = vb;
          pairs[b] = va;
        }
      }
      __syncthreads();
    }
  }
  const long col = (long)d * S;
  for (int p = t; p < S; p += KNN_ST) {
    const unsigned long long v = pairs[p];
    vals[col + p] = value_of((uint32_t)(v >> 32));
    idx[col + p] = (int32_t)(uint32_t)v;
  }
}

// is a distance inside the radius: strictly below it, or 0 where the radius is 0
__device__ __forceinline__ bool inside(double dist, double radius) { return radius > 0. ? dist < radius : dist <= 0.; }

__global__ __launch_bounds__(KNN_T) void k_knn_mi(const int64_t* __restrict__ rows, Factors fac, int D, int K, int S, int kn, int sum_sizes,
                                                  const double* __restrict__ psi, const float* __restrict__ vals,
                                                  const int32_t* __restrict__ idx, double* __restrict__ sums,
                                                  int32_t* __restrict__ class_counts, int32_t* __restrict__ m_of,
                                                  int32_t* __restrict__ k_of) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ MiTables f;
  float* xs = (float*)lds;                                       // [S] the sorted values; after the split the n kept ones
  uint16_t* cq = (uint16_t*)(xs + S);                            // [S] the class lists one after another: places in xs
  uint16_t* sidx = cq + S;                                       // [S] the selection index of xs[.]
  uint8_t* lab = (uint8_t*)(sidx + S);                           // [S] the label of xs[.]
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int k = blockIdx.x, d = blockIdx.y;
  int size = 1, off = 0;
  long stride = 1;
#pragma unroll
  for (int j = 0; j < DVAE_KNN_MAX_FACTORS; ++j) {               // the same in every thread
    if (j == k) {
      size = fac.size[j];
      off = fac.offset[j];
      stride = fac.stride[j];
    }
  }
  for (int i = t; i < KNN_C; i += KNN_T) f.cnt[i] = 0;
  for (int i = t; i < KNN_WAVES * KNN_C; i += KNN_T) f.wave_cnt[i] = 0;
  __syncthreads();

  // ---- load: the sorted column, the labels from the row numbers, the class counts
  const long col = (long)d * S;
  for (int p = t; p < S; p += KNN_T) {
    int si = idx[col + p];
    if ((unsigned)si >= (unsigned)S) si = 0;                     // (a workspace that dvae_knn_sort did not write: stay inside `rows`)
    const unsigned long row = rows ? (unsigned long)rows[si] : (unsigned long)si;
    const int v = (int)((row / (unsigned long)stride) % (unsigned long)size);
    xs[p] = vals[col + p];
    sidx[p] = (uint16_t)si;
    lab[p] = (uint8_t)v;
    atomicAdd(&f.cnt[v], 1);                                     // an INTEGER add in LDS: the order does not show
  }
  __syncthreads();
  if (d == 0) {
    for (int e = t; e < sum_sizes; e += KNN_T) class_counts[(long)k * sum_sizes + e] = e >= off && e < off + size ? f.cnt[e - off] : 0;
  }
  {                                                              // the starts of the class lists: an exclusive scan of the kept counts
    const int rows_of_class = t < KNN_C ? f.cnt[t] : 0, c = rows_of_class >= 2 ? rows_of_class : 0;
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int nb = __shfl_up(incl, o, 64);
      if (lane >= o) incl += nb;
    }
    if (lane == 63) f.wave_keep[w] = incl;
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int i = 0; i < KNN_WAVES; ++i)
      if (i < w) before += f.wave_keep[i];
    if (t < KNN_C) {
      f.cstart[t] = before + incl - c;
      f.cpos[t] = before + incl - c;
    }
    __syncthreads();
  }

  // ---- split: the stable compaction and the stable partition by class, one pass
  const long dump = ((long)d * K + k) * S;
  int n = 0;                                                     // kept rows so far (the same in every thread)
  for (int base = 0; base < S; base += KNN_T) {                  // the same trip count in every thread: barriers inside
    const int p = base + t;
    const bool valid = p < S;
    int v = 0, si = 0;
    float x = 0.f;
    if (valid) {
      v = lab[p];
      si = sidx[p];
      x = xs[p];
    }
    const bool keep = valid && f.cnt[v] >= 2;
    const unsigned long long same = same_digit((uint32_t)v, keep), kept = __ballot(keep), lower = (1ull << lane) - 1ull;
    const int rank = __popcll(same & lower), krank = __popcll(kept & lower);
    if (keep && rank == 0) f.wave_cnt[w * KNN_C + v] = __popcll(same);
    if (lane == 0) f.wave_keep[w] = __popcll(kept);
    __syncthreads();                                             // and every read of this tile is done
    int tile_kept = 0;
#pragma unroll
    for (int i = 0; i < KNN_WAVES; ++i) tile_kept += f.wave_keep[i];
    if (keep) {
      int j = f.cpos[v] + rank, q = n + krank;
#pragma unroll
      for (int i = 0; i < KNN_WAVES; ++i) {
        if (i < w) {
          j += f.wave_cnt[i * KNN_C + v];
          q += f.wave_keep[i];
        }
      }
      xs[q] = x;                                                 // q <= p: a place this tile or an earlier one has read
      sidx[q] = (uint16_t)si;
      lab[q] = (uint8_t)v;
      cq[j] = (uint16_t)q;
    } else if (valid) {                                          // the only row of its class: dropped
      if (m_of) m_of[dump + si] = 0;
      if (k_of) k_of[dump + si] = 0;
    }
    n += tile_kept;
    __syncthreads();
    if (t < KNN_C) {
      int add = 0;
#pragma unroll
      for (int i = 0; i < KNN_WAVES; ++i) {
        add += f.wave_cnt[i * KNN_C + t];
        f.wave_cnt[i * KNN_C + t] = 0;
      }
      f.cpos[t] += add;
    }
    __syncthreads();
  }

  // ---- walk, search, sum
  double sk = 0., sc = 0., sm = 0.;
  for (int j = t; j < n; j += KNN_T) {
    const int q = cq[j], v = lab[q];
    const double x = (double)xs[q];
    const int c = f.cnt[v], lo = f.cstart[v], hi = lo + c;       // this class list is cq[lo .. hi), lo <= j < hi
    const int kk = c - 1 < kn ? c - 1 : kn;                      // >= 1
    int l = j - 1, r = j + 1;
    double radius = 0.;
    for (int s = 0; s < kk; ++s) {                               // kk <= c - 1 others: one side is always there
      const double dl = l >= lo ? x - (double)xs[cq[l]] : (double)INFINITY;
      const double dr = r < hi ? (double)xs[cq[r]] - x : (double)INFINITY;
      if (dl <= dr) {
        radius = dl;
        --l;
      } else {
        radius = dr;
        ++r;
      }
    }
    int a = 0, b = q;                                            // the first place whose distance is inside: in [a, b]; q itself is
#pragma unroll 1
    for (int it = 0; it < KNN_BISECT; ++it) {
      if (a < b) {
        const int mid = (a + b) >> 1;
        if (inside(x - (double)xs[mid], radius)) b = mid; else a = mid + 1;
      }
    }
    int a2 = q, b2 = n - 1;                                      // the last such place: in [a2, b2]
#pragma unroll 1
    for (int it = 0; it < KNN_BISECT; ++it) {
      if (a2 < b2) {
        const int mid = (a2 + b2 + 1) >> 1;
        if (inside((double)xs[mid] - x, radius)) a2 = mid; else b2 = mid - 1;
      }
    }
    const int m = a2 - a + 1;                                    // in [1, n]
    sk += psi[kk];
    sc += psi[c];
    sm += psi[m];
    if (m_of) m_of[dump + sidx[q]] = m;
    if (k_of) k_of[dump + sidx[q]] = kk;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    sk += __shfl_down(sk, o, 64);
    sc += __shfl_down(sc, o, 64);
    sm += __shfl_down(sm, o, 64);
  }
  if (lane == 0) {
    f.red[w * 3] = sk;
    f.red[w * 3 + 1] = sc;
    f.red[w * 3 + 2] = sm;
  }
  __syncthreads();
  if (t == 0) {
    double a0 = f.red[0], a1 = f.red[1], a2 = f.red[2];
#pragma unroll
    for (int i = 1; i < KNN_WAVES; ++i) {
      a0 += f.red[i * 3];
      a1 += f.red[i * 3 + 1];
      a2 += f.red[i * 3 + 2];
    }
    double* out = sums + ((long)d * K + k) * 4;
    out[0] = (double)n;
    out[1] = a0;
    out[2] = a1;
    out[3] = a2;
  }
}

// the K factors -> sum(lat_sizes) with the strides and offsets filled in, or -1; *rows_enumerated = prod(lat_sizes), capped above 2^31
long load_factors(const int32_t* lat_sizes, int K, Factors* f, long* rows_enumerated) {
  if (!lat_sizes || K < 1 || K > DVAE_KNN_MAX_FACTORS) return -1;
  long sum = 0;
  for (int j = 0; j < DVAE_KNN_MAX_FACTORS; ++j) {
    f->size[j] = j < K ? lat_sizes[j] : 1;
    if (f->size[j] < 1 || f->size[j] > DVAE_KNN_MAX_CLASSES) return -1;
    f->offset[j] = (int)sum;
    if (j < K) sum += f->size[j];
  }
  long prod = 1;
  for (int j = DVAE_KNN_MAX_FACTORS - 1; j >= 0; --j) {
    f->stride[j] = prod;
    if (prod <= 2147483647L) prod *= f->size[j];                 // beyond 2^31 the product only has to stay too large
  }
  *rows_enumerated = prod;
  return sum;
}

bool sizes_ok(long N, int D, long S) {
  return N >= 1 && N <= 2147483647L && D >= 1 && D <= DVAE_KNN_MAX_D && S >= 1 && S <= DVAE_KNN_MAX_ROWS;
}

// more than 64 KiB of dynamic LDS must be asked for, once per device
template <typename Kernel>
int allow_lds(DeviceOnce* once, Kernel kernel, int bytes, const char* file, int line) {
  if (once->first() && hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s:%d: the device refuses %d bytes of LDS per workgroup", file, line, bytes);
    return -2;
  }
  return 0;
}

}  // namespace
}  // namespace dvae

using namespace dvae;

extern "C" {

int dvae_knn_version(void) { return DVAE_KNN_VERSION; }
const char* dvae_knn_last_error(void) { return last_error(); }

size_t dvae_knn_ws_bytes(long N, int D, long S) {
  if (S <= 0) S = N;
  if (!sizes_ok(N, D, S)) return 0;
  return (size_t)(8L * D * S);
}

int dvae_knn_sort(const float* table, const int64_t* rows, long N, int D, long S, void* ws, void* stream) {
  if (!rows) S = N;
  DVAE_CHECK_ARG(table && ws);
  DVAE_CHECK_ARG(N >= 1 && N <= 2147483647L);
  DVAE_CHECK_ARG(D >= 1 && D <= DVAE_KNN_MAX_D);
  DVAE_CHECK_ARG(S >= 1 && S <= DVAE_KNN_MAX_ROWS);
  int P2 = 1;
  for (int b = 0; b < 31 && P2 < S; ++b) P2 <<= 1;               // the column padded to a power of two: <= DVAE_KNN_MAX_ROWS
  static DeviceOnce attr;
  const int rc = allow_lds(&attr, k_knn_sort, DVAE_KNN_SORT_ROW_BYTES * DVAE_KNN_MAX_ROWS, __FILE__, __LINE__);
  if (rc) return rc;
  float* vals = (float*)ws;
  int32_t* idx = (int32_t*)(vals + (long)D * S);
  hipLaunchKernelGGL(k_knn_sort, dim3(D), dim3(KNN_ST), (size_t)DVAE_KNN_SORT_ROW_BYTES * P2, (hipStream_t)stream, table, rows, D, (int)S, P2,
                     vals, idx);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int dvae_knn_mi(const int64_t* rows, const int32_t* lat_sizes, long N, int D, int K, long S, int n_neighbors, const double* psi,
                const void* ws, double* sums, int32_t* class_counts, int32_t* m_of, int32_t* k_of, void* stream) {
  if (!rows) S = N;
  DVAE_CHECK_ARG(lat_sizes && psi && ws && sums && class_counts);
  DVAE_CHECK_ARG(N >= 1 && N <= 2147483647L);
  DVAE_CHECK_ARG(D >= 1 && D <= DVAE_KNN_MAX_D);
  DVAE_CHECK_ARG(K >= 1 && K <= DVAE_KNN_MAX_FACTORS);
  DVAE_CHECK_ARG(S >= 1 && S <= DVAE_KNN_MAX_ROWS);
  DVAE_CHECK_ARG(n_neighbors >= 1 && n_neighbors <= DVAE_KNN_MAX_NEIGHBORS);
  Factors fac;
  long rows_enumerated = 0;
  const long sum_sizes = load_factors(lat_sizes, K, &fac, &rows_enumerated);
  DVAE_CHECK_ARG(sum_sizes >= 1);
  DVAE_CHECK_ARG(rows_enumerated == N);
  static DeviceOnce attr;
  const int rc = allow_lds(&attr, k_knn_mi, DVAE_KNN_MI_ROW_BYTES * DVAE_KNN_MAX_ROWS, __FILE__, __LINE__);
  if (rc) return rc;
  const float* vals = (const float*)ws;
  const int32_t* idx = (const int32_t*)(vals + (long)D * S);
  hipLaunchKernelGGL(k_knn_mi, dim3(K, D), dim3(KNN_T), (size_t)DVAE_KNN_MI_ROW_BYTES * S, (hipStream_t)stream, rows, fac, D, K, (int)S,
                     n_neighbors, (int)sum_sizes, psi, vals, idx, sums, class_counts, m_of, k_of);
  DVAE_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
