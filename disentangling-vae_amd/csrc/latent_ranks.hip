// libdvae_udr_hip.so (include/dvae_udr_hip.h): what the unsupervised disentanglement ranking (Duan et al. 2020) needs of a model's
// [N, D] tables of posterior means and log-variances over S selected rows -- the tie-averaged rank of every element within its
// column (the Spearman correlation of two models' latents is the Pearson correlation of these) and the mean KL divergence of
// every latent dimension from the prior.
//
// Ranks.  A value becomes a 32-bit key whose unsigned order is the numeric order of the floats (sign flipped for positives, all
// bits for negatives, -0 folded into +0 first; bit operations only, so denormals stay what they are).  (key, s) is sorted per
// column by an LSD radix sort, four passes of 8-bit digits.  Above DVAE_UDR_SMALL_ROWS a pass is three launches:
//   k_udr_count    a workgroup per (chunk, column) counts the digits of its chunk in LDS -> hist[column][digit][chunk];
//   k_udr_offsets  a workgroup per column, a thread per digit: the exclusive scan of hist in (digit, chunk) order;
//   k_udr_scatter  a workgroup per (chunk, column) walks its chunk in tiles of 256 in order.  A wave finds the lanes of equal
//                  digit with eight 64-bit ballots: a lane's rank among them is a population count below it, and their leader
//                  publishes their number in wave_cnt[wave][digit].  After a barrier a lane's place is the running offset of
//                  its digit plus the numbers of the waves before its own plus its rank; then thread t adds the four waves'
//                  numbers of digit t to the running offset.  Integer adds only; equal digits keep their order (stable).
// The first pass reads the table (through `rows`) and makes the keys; the others read the ping-pong buffer the pass before
// wrote.  No workgroup waits on another: the launch boundary is the only ordering.  The count needs the same ballots as the
// scatter -- one LDS add per distinct digit of a wave, whatever the data: a collapsed latent (every key equal) or the
// exponent byte of a Gaussian column would otherwise queue all 64 lanes on one LDS address.
// Runs of equal keys.  Position p of a sorted column starts a run when p = 0 or key[p - 1] differs, and ends one when p = S - 1 or
// key[p + 1] differs.  first[p] is the inclusive maximum scan of (p if start), last[p] the inclusive minimum scan from the right
// of (p if end): k_udr_runs_first sweeps a chunk's tiles forwards, stores first[p] (or -1: no start in this chunk so far) into the
// idle key buffer and records the chunk's last start and first end; k_udr_runs_ranks takes the last start of the chunks before
// and the first end of the chunks after its own (a run may span every chunk: a collapsed latent is one run of length S), sweeps
// the tiles backwards and stores (first + last) / 2 + 1 to ranks[s, d].  Every loop bound is a function of the arguments.
// Up to DVAE_UDR_SMALL_ROWS rows k_udr_ranks_small does all of it for a column in one workgroup, the buffers in LDS, with the
// same device functions.
// Loads are one 32-bit word per lane: ws, table and ranks are promised at 4-byte alignment and no more.
//
// KL.  A thread per (chunk of rows, latent) -- padded_width(D) lanes per row, so the lanes of a row read consecutive floats -- walks
// the rows of its chunk in order and adds 0.5 (mu^2 + exp(lv) - lv - 1) in an fp64 register, every float converted first; one
// record of D doubles per chunk.  The chunks are short (DVAE_UDR_KL_BLOCK_ROWS) and many (DVAE_UDR_KL_MAX_CHUNKS): the sum in
// order is one thread's work, so the parallelism is in their number.  k_udr_kl_finish, a wave per latent, adds the records in
// the order of the chunks: 64 at a time are loaded by the 64 lanes and handed round by lane shuffles.
#include <limits.h>

#include "../../include/dvae_udr_hip.h"
#include "common.h"
#include "last_error.h"
#include "table_stats.h"

namespace dvae {

namespace {

#define UDR_T 256
#define UDR_WAVES (UDR_T / 64)
#define UDR_DIGITS 256
#define UDR_PASSES 4

static_assert(UDR_DIGITS == UDR_T, "thread t owns digit t");
static_assert(DVAE_UDR_MAX_CHUNKS <= UDR_T, "k_udr_runs_ranks reads one chunk record per thread");
static_assert(DVAE_UDR_MAX_ROWS <= (1L << 23), "first + last + 2 <= 2^24 must be an fp32 integer");
static_assert(DVAE_UDR_MAX_D <= 64, "padded_width(D) lanes hold a row in the KL pass");

// unsigned order of the key = numeric order of the float; -0 and +0 give one key
__device__ __forceinline__ uint32_t key_of(float x) {
  uint32_t u = __float_as_uint(x);
  if ((u << 1) == 0u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
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

// inclusive scans over the 256 threads of the workgroup, and the value of the whole workgroup; scratch: UDR_WAVES ints
__device__ __forceinline__ int block_scan_max(int v, int* scratch, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int n = __shfl_up(v, o, 64);
    if (lane >= o) v = max(v, n);
  }
  if (lane == 63) scratch[w] = v;
  __syncthreads();
  int all = INT_MIN;
#pragma unroll
  for (int i = 0; i < UDR_WAVES; ++i) {
    if (i < w) v = max(v, scratch[i]);
    all = max(all, scratch[i]);
  }
  __syncthreads();                                           // scratch is free again
  *total = all;
  return v;
}
__device__ __forceinline__ int block_scan_add(int v, int* scratch) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int n = __shfl_up(v, o, 64);
    if (lane >= o) v += n;
  }
  if (lane == 63) scratch[w] = v;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < UDR_WAVES; ++i)
    if (i < w) v += scratch[i];
  __syncthreads();
  return v;
}

// element p of column d: its key and the number of its row within the selection
template <bool FIRST>
__device__ __forceinline__ void load_pair(const float* __restrict__ table, const int64_t* __restrict__ rows, int D, int d,
                                          const uint32_t* src_key, const uint32_t* src_idx, long p, uint32_t* key, uint32_t* idx) {
  if (FIRST) {
    const long row = rows ? (long)rows[p] : p;
    *key = key_of(table[row * D + d]);
    *idx = (uint32_t)p;
  } else {
    *key = src_key[p];
    *idx = src_idx[p];
  }
}

// digits of positions [c0, c1) added to cnt[UDR_DIGITS] (LDS, cleared by the caller): one add per distinct digit of a wave
template <bool FIRST>
__device__ __forceinline__ void count_digits(const float* __restrict__ table, const int64_t* __restrict__ rows, int D, int d,
                                             const uint32_t* src_key, long c0, long c1, int shift, int* cnt) {
  const int t = threadIdx.x, lane = t & 63;
  for (long base = c0; base < c1; base += UDR_T) {
    const long p = base + t;
    const bool valid = p < c1;
    uint32_t key = 0, idx = 0;
    if (valid) load_pair<FIRST>(table, rows, D, d, src_key, src_key, p, &key, &idx);
    const uint32_t digit = (key >> shift) & 255u;
    const unsigned long long m = same_digit(digit, valid);
    if (valid && __ffsll((long long)m) - 1 == lane) atomicAdd(&cnt[digit], __popcll(m));
  }
}

// stable scatter of positions [c0, c1) by digit.  cnt[UDR_DIGITS]: where the next element of every digit goes (LDS, set by the
// caller, a barrier since); wave_cnt[UDR_WAVES * UDR_DIGITS]: LDS, zero on entry and on return.
template <bool FIRST>
__device__ __forceinline__ void scatter_digits(const float* __restrict__ table, const int64_t* __restrict__ rows, int D, int d,
                                               const uint32_t* src_key, const uint32_t* src_idx, uint32_t* dst_key,
                                               uint32_t* dst_idx, long c0, long c1, int shift, int* cnt, int* wave_cnt) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (long base = c0; base < c1; base += UDR_T) {           // the same trip count in every thread: barriers inside
    const long p = base + t;
    const bool valid = p < c1;
    uint32_t key = 0, idx = 0;
    if (valid) load_pair<FIRST>(table, rows, D, d, src_key, src_idx, p, &key, &idx);
    const uint32_t digit = (key >> shift) & 255u;
    const unsigned long long m = same_digit(digit, valid);
    const int rank = __popcll(m & ((1ull << lane) - 1ull));
    if (valid && rank == 0) wave_cnt[w * UDR_DIGITS + digit] = __popcll(m);
    __syncthreads();
    if (valid) {
      int pos = cnt[digit] + rank;
#pragma unroll
      for (int i = 0; i < UDR_WAVES - 1; ++i)
        if (i < w) pos += wave_cnt[i * UDR_DIGITS + digit];
      dst_key[pos] = key;
      dst_idx[pos] = idx;
    }
    __syncthreads();
    int add = 0;
#pragma unroll
    for (int i = 0; i < UDR_WAVES; ++i) {
      add += wave_cnt[i * UDR_DIGITS + t];
      wave_cnt[i * UDR_DIGITS + t] = 0;
    }
    cnt[t] += add;
    __syncthreads();
  }
}

// forward sweep over positions [c0, c1) of a sorted column of S keys: first[p] = the last run start in [c0, p], or -1.
// -> the last start and the first end of [c0, c1) (-1 / INT_MAX: none), the same in every thread
__device__ __forceinline__ void sweep_first(const uint32_t* key, uint32_t* first, long c0, long c1, long S, int* scratch,
                                            int* last_start, int* first_end) {
  const int t = threadIdx.x;
  int carry = -1, end_min = INT_MAX;
  for (long base = c0; base < c1; base += UDR_T) {
    const long p = base + t;
    int v = -1;
    if (p < c1) {
      const uint32_t k = key[p];
      if (p == 0 || key[p - 1] != k) v = (int)p;
      if (p == S - 1 || key[p + 1] != k) end_min = min(end_min, (int)p);
    }
    int total;
    v = max(block_scan_max(v, scratch, &total), carry);
    if (p < c1) first[p] = (uint32_t)v;
    carry = max(carry, total);
  }
  int neg_end;
  block_scan_max(-end_min, scratch, &neg_end);
  *last_start = carry;
  *first_end = -neg_end;
}

// backward sweep: last[p] = the first run end in [p, c1) or `end_after`; first[p] < 0 stands for `start_before`
__device__ __forceinline__ void sweep_ranks(const uint32_t* key, const uint32_t* first, const uint32_t* idx, long c0, long c1, long S,
                                            int start_before, int end_after, int D, int d, float* __restrict__ ranks, int* scratch) {
  const int t = threadIdx.x;
  const long tiles = (c1 - c0 + UDR_T - 1) / UDR_T;
  int carry = -end_after;                                    // a minimum scan as the maximum scan of the negated positions
  for (long j = tiles - 1; j >= 0; --j) {
    const long p = c0 + j * UDR_T + (UDR_T - 1 - t);         // thread 0 takes the tile's last position
    int v = -INT_MAX;
    if (p < c1) {
      const uint32_t k = key[p];
      if (p == S - 1 || key[p + 1] != k) v = -(int)p;
    }
    int total;
    v = max(block_scan_max(v, scratch, &total), carry);
    if (p < c1) {
      int f = (int)first[p];
      if (f < 0) f = start_before;
      ranks[(long)idx[p] * D + d] = 0.5f * (float)(f - v + 2);   // (first + last) / 2 + 1: first + last + 2 <= 2^24, exact
    }
    carry = max(carry, total);
  }
}

// ---- ranks: the chunked path ----------------------------------------------------------------------------------------------------
struct UdrWs {                                               // the workspace in 32-bit words
  uint32_t *key[2], *idx[2];                                 // [D, S] each
  int *hist;                                                 // [D, UDR_DIGITS, nchunks]
  int *last_start, *first_end;                               // [D, nchunks] each
};
__host__ __device__ __forceinline__ UdrWs udr_ws(float* ws, int D, long S, int nchunks) {
  UdrWs u;
  uint32_t* p = (uint32_t*)ws;
  const long col = (long)D * S;
  u.key[0] = p;
  u.idx[0] = p + col;
  u.key[1] = p + 2 * col;
  u.idx[1] = p + 3 * col;
  u.hist = (int*)(p + 4 * col);
  u.last_start = u.hist + (long)D * UDR_DIGITS * nchunks;
  u.first_end = u.last_start + (long)D * nchunks;
  return u;
}
size_t udr_ws_words(int D, long S, int nchunks) {
  return (size_t)(4L * D * S + (long)D * UDR_DIGITS * nchunks + 2L * D * nchunks);
}

template <bool FIRST>
__global__ __launch_bounds__(UDR_T) void k_udr_count(const float* __restrict__ table, const int64_t* __restrict__ rows, int D, long S,
                                                     long chunk, int nchunks, int pass, float* ws) {
  __shared__ int cnt[UDR_DIGITS];
  const int t = threadIdx.x, c = blockIdx.x, d = blockIdx.y;
  const UdrWs u = udr_ws(ws, D, S, nchunks);
  const long c0 = c * chunk, c1 = lesser(S, c0 + chunk);
  cnt[t] = 0;
  __syncthreads();
  count_digits<FIRST>(table, rows, D, d, u.key[(pass + 1) & 1] + (long)d * S, c0, c1, 8 * pass, cnt);
  __syncthreads();
  u.hist[((long)d * UDR_DIGITS + t) * nchunks + c] = cnt[t];
}

__global__ __launch_bounds__(UDR_T) void k_udr_offsets(int D, long S, int nchunks, float* ws) {
  __shared__ int scratch[UDR_WAVES];
  const int t = threadIdx.x, d = blockIdx.x;
  const UdrWs u = udr_ws(ws, D, S, nchunks);
  int* line = u.hist + ((long)d * UDR_DIGITS + t) * nchunks;  // digit t of column d, every chunk
  int sum = 0;
  for (int c = 0; c < nchunks; ++c) sum += line[c];
  int at = block_scan_add(sum, scratch) - sum;               // the keys of smaller digits
  for (int c = 0; c < nchunks; ++c) {
    const int n = line[c];
    line[c] = at;
    at += n;
  }
}

template <bool FIRST>
__global__ __launch_bounds__(UDR_T) void k_udr_scatter(const float* __restrict__ table, const int64_t* __restrict__ rows, int D,
                                                       long S, long chunk, int nchunks, int pass, float* ws) {
  __shared__ int cnt[UDR_DIGITS];
  __shared__ int wave_cnt[UDR_WAVES * UDR_DIGITS];
  const int t = threadIdx.x, c = blockIdx.x, d = blockIdx.y;
  const UdrWs u = udr_ws(ws, D, S, nchunks);
  const long c0 = c * chunk, c1 = lesser(S, c0 + chunk), col = (long)d * S;
  const int from = (pass + 1) & 1, to = pass & 1;
  cnt[t] = u.hist[((long)d * UDR_DIGITS + t) * nchunks + c];
#pragma unroll
  for (int i = 0; i < UDR_WAVES; ++i) wave_cnt[i * UDR_DIGITS + t] = 0;
  __syncthreads();
  scatter_digits<FIRST>(table, rows, D, d, u.key[from] + col, u.idx[from] + col, u.key[to] + col, u.idx[to] + col, c0, c1, 8 * pass,
                        cnt, wave_cnt);
}

// after UDR_PASSES passes the sorted column lies in buffer (UDR_PASSES - 1) & 1; the keys of the other one are idle
#define UDR_SORTED ((UDR_PASSES - 1) & 1)

__global__ __launch_bounds__(UDR_T) void k_udr_runs_first(int D, long S, long chunk, int nchunks, float* ws) {
  __shared__ int scratch[UDR_WAVES];
  const int c = blockIdx.x, d = blockIdx.y;
  const UdrWs u = udr_ws(ws, D, S, nchunks);
  const long c0 = c * chunk, c1 = lesser(S, c0 + chunk), col = (long)d * S;
  int last_start, first_end;
  sweep_first(u.key[UDR_SORTED] + col, u.key[UDR_SORTED ^ 1] + col, c0, c1, S, scratch, &last_start, &first_end);
  if (threadIdx.x == 0) {
    u.last_start[(long)d * nchunks + c] = last_start;
    u.first_end[(long)d * nchunks + c] = first_end;
  }
}

__global__ __launch_bounds__(UDR_T) void k_udr_runs_ranks(int D, long S, long chunk, int nchunks, float* ws, float* __restrict__ ranks) {
  __shared__ int scratch[UDR_WAVES];
  const int t = threadIdx.x, c = blockIdx.x, d = blockIdx.y;
  const UdrWs u = udr_ws(ws, D, S, nchunks);
  const long c0 = c * chunk, c1 = lesser(S, c0 + chunk), col = (long)d * S;
  // thread t reads chunk t: the last start before this chunk, the first end after it (position 0 starts a run, S - 1 ends one)
  int before, after;
  block_scan_max(t < c ? u.last_start[(long)d * nchunks + t] : -1, scratch, &before);
  block_scan_max(t > c && t < nchunks ? -u.first_end[(long)d * nchunks + t] : -INT_MAX, scratch, &after);
  sweep_ranks(u.key[UDR_SORTED] + col, u.key[UDR_SORTED ^ 1] + col, u.idx[UDR_SORTED] + col, c0, c1, S, before, -after, D, d, ranks,
              scratch);
}

// ---- ranks: a column in one workgroup ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(UDR_T) void k_udr_ranks_small(const float* __restrict__ table, const int64_t* __restrict__ rows, int D,
                                                           int S, float* __restrict__ ranks) {
  __shared__ uint32_t key[2][DVAE_UDR_SMALL_ROWS], idx[2][DVAE_UDR_SMALL_ROWS];
  __shared__ int cnt[UDR_DIGITS];
  __shared__ int wave_cnt[UDR_WAVES * UDR_DIGITS];
  __shared__ int scratch[UDR_WAVES];
  const int t = threadIdx.x, d = blockIdx.x;
  for (int p = t; p < S; p += UDR_T) load_pair<true>(table, rows, D, d, nullptr, nullptr, p, &key[0][p], &idx[0][p]);
#pragma unroll
  for (int i = 0; i < UDR_WAVES; ++i) wave_cnt[i * UDR_DIGITS + t] = 0;
  for (int pass = 0; pass < UDR_PASSES; ++pass) {            // buffer 0 -> 1 -> 0 -> 1 -> 0
    const int from = pass & 1, to = from ^ 1;
    cnt[t] = 0;
    __syncthreads();                                         // and the keys of `from` are written
    count_digits<false>(table, rows, D, d, key[from], 0, S, 8 * pass, cnt);
    __syncthreads();
    const int n = cnt[t];
    const int at = block_scan_add(n, scratch) - n;
    cnt[t] = at;
    __syncthreads();
    scatter_digits<false>(table, rows, D, d, key[from], idx[from], key[to], idx[to], 0, S, 8 * pass, cnt, wave_cnt);
  }
  static_assert(UDR_PASSES % 2 == 0, "the sorted column is back in buffer 0");
  int last_start, first_end;
  sweep_first(key[0], key[1], 0, S, S, scratch, &last_start, &first_end);
  __syncthreads();
  sweep_ranks(key[0], key[1], idx[0], 0, S, S, 0, S - 1, D, d, ranks, scratch);
}

// ---- KL per dimension ----------------------------------------------------------------------------------------------------------
// thread t of a workgroup: latent t % W of chunk blockIdx.x * (UDR_T / W) + t / W, W = padded_width(D) lanes per row
__global__ __launch_bounds__(UDR_T) void k_udr_kl_part(const float* __restrict__ mean, const float* __restrict__ logvar,
                                                       const int64_t* __restrict__ rows, int D, int W, long S, long chunk, int nb,
                                                       float* __restrict__ ws) {
  const int d = threadIdx.x % W;
  const long b = (long)blockIdx.x * (UDR_T / W) + threadIdx.x / W;
  if (d >= D || b >= nb) return;
  const long c0 = b * chunk, c1 = lesser(S, c0 + chunk);
  double acc = 0.;
  for (long s = c0; s < c1; ++s) {
    const long row = rows ? (long)rows[s] : s;
    const double mu = (double)mean[row * D + d], lv = (double)logvar[row * D + d];
    acc += 0.5 * (mu * mu + exp(lv) - lv - 1.);
  }
  put_f64(ws + 2 * (b * D + d), acc);
}

// a wave per latent: 64 records at a time are loaded by the 64 lanes and added in the order of the chunks
__global__ __launch_bounds__(64) void k_udr_kl_finish(int D, long S, int nb, const float* __restrict__ ws, double* __restrict__ kl) {
  const int d = blockIdx.x, lane = threadIdx.x;
  double acc = 0.;
  for (int b0 = 0; b0 < nb; b0 += 64) {
    const int b = b0 + lane, n = lesser(64, nb - b0);
    const double v = b < nb ? get_f64(ws + 2 * ((long)b * D + d)) : 0.;
#pragma unroll 8
    for (int i = 0; i < 64; ++i) {
      const double x = __shfl(v, i, 64);
      if (i < n) acc += x;
    }
  }
  if (lane == 0) kl[d] = acc / (double)S;
}

bool sizes_ok(long N, int D, long S, long max_rows) {
  return N > 0 && N <= 2147483647L && D > 0 && D <= DVAE_UDR_MAX_D && S > 0 && S <= max_rows;
}

}  // namespace
}  // namespace dvae

using namespace dvae;

extern "C" {

int dvae_udr_version(void) { return DVAE_UDR_VERSION; }
const char* dvae_udr_last_error(void) { return last_error(); }

size_t dvae_udr_ranks_ws_floats(long N, int D, long S) {
  if (S <= 0) S = N;
  if (!sizes_ok(N, D, S, DVAE_UDR_MAX_ROWS)) return 0;
  if (S <= DVAE_UDR_SMALL_ROWS) return 1;                      // everything in LDS
  long chunk;
  const int nchunks = chunks_of(S, DVAE_UDR_CHUNK_ROWS, DVAE_UDR_MAX_CHUNKS, &chunk);
  return udr_ws_words(D, S, nchunks);
}

size_t dvae_udr_kl_dims_ws_floats(long N, int D, long S) {
  if (S <= 0) S = N;
  if (!sizes_ok(N, D, S, 2147483647L)) return 0;
  long chunk;
  const int nb = chunks_of(S, DVAE_UDR_KL_BLOCK_ROWS, DVAE_UDR_KL_MAX_CHUNKS, &chunk);
  return (size_t)(2L * nb * D);                                // a double per (chunk, latent)
}

int dvae_udr_ranks(const float* table, const int64_t* rows, long N, int D, long S, float* ws, float* ranks, void* stream) {
  if (!rows) S = N;
  DVAE_CHECK_ARG(table && ws && ranks);
  DVAE_CHECK_ARG(D <= DVAE_UDR_MAX_D);
  DVAE_CHECK_ARG(S <= DVAE_UDR_MAX_ROWS);
  DVAE_CHECK_ARG(sizes_ok(N, D, S, DVAE_UDR_MAX_ROWS));
  hipStream_t st = (hipStream_t)stream;
  if (S <= DVAE_UDR_SMALL_ROWS) {
    hipLaunchKernelGGL(k_udr_ranks_small, dim3(D), dim3(UDR_T), 0, st, table, rows, D, (int)S, ranks);
    DVAE_CHECK_LAUNCH();
    return 0;
  }
  long chunk;
  const int nchunks = chunks_of(S, DVAE_UDR_CHUNK_ROWS, DVAE_UDR_MAX_CHUNKS, &chunk);
  const dim3 grid(nchunks, D), block(UDR_T);
  for (int pass = 0; pass < UDR_PASSES; ++pass) {
    if (pass == 0)
      hipLaunchKernelGGL(k_udr_count<true>, grid, block, 0, st, table, rows, D, S, chunk, nchunks, pass, ws);
    else
      hipLaunchKernelGGL(k_udr_count<false>, grid, block, 0, st, table, rows, D, S, chunk, nchunks, pass, ws);
    DVAE_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_udr_offsets, dim3(D), block, 0, st, D, S, nchunks, ws);
    DVAE_CHECK_LAUNCH();
    if (pass == 0)
      hipLaunchKernelGGL(k_udr_scatter<true>, grid, block, 0, st, table, rows, D, S, chunk, nchunks, pass, ws);
    else
      hipLaunchKernelGGL(k_udr_scatter<false>, grid, block, 0, st, table, rows, D, S, chunk, nchunks, pass, ws);
    DVAE_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_udr_runs_first, grid, block, 0, st, D, S, chunk, nchunks, ws);
  DVAE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_udr_runs_ranks, grid, block, 0, st, D, S, chunk, nchunks, ws, ranks);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int dvae_udr_kl_dims(const float* mean, const float* logvar, const int64_t* rows, long N, int D, long S, float* ws, double* kl,
                     void* stream) {
  if (!rows) S = N;
  DVAE_CHECK_ARG(mean && logvar && ws && kl);
  DVAE_CHECK_ARG(D <= DVAE_UDR_MAX_D);
  DVAE_CHECK_ARG(sizes_ok(N, D, S, 2147483647L));
  hipStream_t st = (hipStream_t)stream;
  long chunk;
  const int nb = chunks_of(S, DVAE_UDR_KL_BLOCK_ROWS, DVAE_UDR_KL_MAX_CHUNKS, &chunk);
  const int W = padded_width(D), per_group = UDR_T / W;
  hipLaunchKernelGGL(k_udr_kl_part, dim3((nb + per_group - 1) / per_group), dim3(UDR_T), 0, st, mean, logvar, rows, D, W, S, chunk, nb, ws);
  DVAE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_udr_kl_finish, dim3(D), dim3(64), 0, st, D, S, nb, ws, kl);
  DVAE_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
