// libdvae_semi_hip.so (include/dvae_semi_hip.h): the supervised regulariser of S2-beta-VAE (Locatello et al. 2020, "Disentangling
// Factors of Variation Using Few Labels") on the labelled rows of a batch of posterior means mu [n, D] -- R (xent / l2 / cov, see
// the header), w dR/dmu -- in two launches.  The shapes are tiny (n D of a million floats at most), so what counts is the number of
// launches and their fixed latency, not bandwidth.  Labels never exist in memory: the value of factor k of row i is
// (rows[i] / stride_k) % size_k, and the K sizes and strides travel as a kernel argument.
//
// k_semi_partials.  The rows are cut into chunks of SEMI_ROWS, one workgroup each.  Thread r < rows of the chunk decodes row r:
// its K values (cov: minus those of the batch's first labelled row, an exact integer difference) go to LDS, zeros for an
// unlabelled row; xent / l2: it adds the row's K terms in the order of k.  Thread 0 then adds the rows' terms and the labelled
// count in the order of the rows.  cov: the chunk's means, shifted by the first labelled row's and converted to fp64 first (so the
// difference is exact; zeros for an unlabelled row), go to LDS, and thread p owns entry p = d K + k (p, p + 256, ...) of the D x K
// cross sum, threads [0, D) the column sums of mu, threads [T / 2, T / 2 + K) those of the values, each over the rows in order.
// One record of 2 + D + K + D K doubles per chunk goes to ws.
//
// k_semi_grad.  One workgroup per chunk again.  Every workgroup adds the records in the order of the chunks -- the same bits of
// n_lab, C and G in all of them -- and keeps G = dR/dC (fp64: D K <= 512 entries) and the shift of the values' mean in LDS;
// workgroup 0 also writes R, n_lab and C to `out` and adds w R to *loss_io.  With dmu the workgroup then walks its rows in fp64,
// one rounding to fp32 at the store; unlabelled rows and (xent / l2) columns >= K receive +0.
//
// The first labelled row of the batch is found by every workgroup of both kernels on its own (n <= 16 384 row numbers, 64 per
// thread): no workgroup waits on another.  No atomics, no cooperative launch; every loop bound is a function of the arguments.
#include "../../include/dvae_semi_hip.h"
#include "common.h"
#include "last_error.h"
#include "table_stats.h"

namespace dvae {

namespace {

#define SEMI_T DVAE_SEMI_THREADS
#define SEMI_ROWS DVAE_SEMI_BLOCK_ROWS
#define SEMI_D DVAE_SEMI_MAX_D
#define SEMI_K DVAE_SEMI_MAX_K

static_assert(SEMI_T == 256 && SEMI_T % 64 == 0, "four waves");
static_assert(SEMI_ROWS <= SEMI_T, "thread r decodes row r of the chunk");
static_assert(SEMI_D <= SEMI_T / 2 && SEMI_K <= SEMI_T / 2, "threads [0, D) add the columns of mu, threads [T / 2, T / 2 + K) those of the values");
static_assert(8 * (SEMI_ROWS * SEMI_D + SEMI_ROWS * SEMI_K + SEMI_ROWS + SEMI_K) + 4 * SEMI_ROWS + 64 <= 64 * 1024, "k_semi_partials' LDS");
static_assert(DVAE_SEMI_MAX_ROWS <= 0x7fffffff / (2 * SEMI_D), "int indices");

// the factors tied to latents 0 .. K - 1: a kernel argument
struct Factors {
  long size[SEMI_K], stride[SEMI_K];
};

// one chunk's record in ws
__host__ __device__ __forceinline__ int rec_doubles(int D, int K) { return 2 + D + K + D * K; }

__device__ __forceinline__ long mu_at(int interleaved, int D, int i, int d) { return interleaved ? 2L * i * D + 2 * d : (long)i * D + d; }

__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int u = __shfl_xor(v, o, 64);
    v = u < v ? u : v;
  }
  return v;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// index of the first labelled row of the batch, n when there is none; `slot`: SEMI_T / 64 ints of LDS.  Ends with a barrier.
__device__ __forceinline__ int first_labelled(const int64_t* __restrict__ rows, int n, int* slot) {
  const int t = threadIdx.x;
  int m = n;
  for (int i = t; i < n; i += SEMI_T)
    if (rows[i] >= 0) {
      m = i;
      break;
    }
  m = wave_min_i32(m);
  if ((t & 63) == 0) slot[t >> 6] = m;
  __syncthreads();
  m = slot[0];
#pragma unroll
  for (int w = 1; w < SEMI_T / 64; ++w) m = slot[w] < m ? slot[w] : m;
  return m;
}

__global__ __launch_bounds__(SEMI_T) void k_semi_partials(const float* __restrict__ mu, int interleaved, const int64_t* __restrict__ rows,
                                                          int n, int D, int K, Factors f, int kind, double* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) double xs[SEMI_ROWS * SEMI_D];   // cov: (mu - mu_0) of the chunk's rows, 0 where unlabelled
  __shared__ double vs[SEMI_ROWS * SEMI_K];                                // cov: v - v_0, 0 where unlabelled
  __shared__ double term[SEMI_ROWS];                                       // xent / l2: the row's part of R
  __shared__ int lab[SEMI_ROWS];
  __shared__ int slot[SEMI_T / 64];
  const int t = threadIdx.x, g = blockIdx.x;
  const int c0 = g * SEMI_ROWS, nr = lesser(SEMI_ROWS, n - c0);
  const bool cov = kind == DVAE_SEMI_COV;
  int i0 = n;
  long row0 = 0;
  if (cov) {
    i0 = first_labelled(rows, n, slot);
    if (i0 < n) row0 = rows[i0];
  }
  if (t < nr) {
    const long row = rows[c0 + t];
    const bool on = row >= 0;
    lab[t] = on;
    double a = 0.;
    for (int k = 0; k < K; ++k) {
      const long v = on ? (row / f.stride[k]) % f.size[k] : 0;
      if (cov) {
        const long v0 = (row0 / f.stride[k]) % f.size[k];
        vs[t * K + k] = on ? (double)(v - v0) : 0.;
      } else if (on) {
        const double x = (double)mu[mu_at(interleaved, D, c0 + t, k)], y = (double)v / (double)f.size[k];
        if (kind == DVAE_SEMI_XENT)
          a += (x > 0. ? x : 0.) - x * y + log1p(exp(-fabs(x)));
        else
          a += (x - y) * (x - y);
      }
    }
    term[t] = a;
  }
  __syncthreads();
  double* rec = ws + (long)g * rec_doubles(D, K);
  if (t == 0) {
    double cnt = 0., a = 0.;
    for (int r = 0; r < nr; ++r) {
      cnt += (double)lab[r];
      a += term[r];
    }
    rec[0] = cnt;
    rec[1] = cov ? 0. : a;
  }
  if (!cov) return;
  for (int i = t; i < nr * D; i += SEMI_T) {
    const int r = i / D, d = i % D;
    xs[i] = lab[r] ? (double)mu[mu_at(interleaved, D, c0 + r, d)] - (double)mu[mu_at(interleaved, D, i0, d)] : 0.;
  }
  __syncthreads();
  for (int p = t; p < D * K; p += SEMI_T) {
    const int d = p / K, k = p % K;
    double a = 0.;
    for (int r = 0; r < nr; ++r) a += xs[r * D + d] * vs[r * K + k];
    rec[2 + D + K + p] = a;
  }
  if (t < D) {
    double a = 0.;
    for (int r = 0; r < nr; ++r) a += xs[r * D + t];
    rec[2 + t] = a;
  }
  if (t >= SEMI_T / 2 && t - SEMI_T / 2 < K) {
    const int k = t - SEMI_T / 2;
    double a = 0.;
    for (int r = 0; r < nr; ++r) a += vs[r * K + k];
    rec[2 + D + k] = a;
  }
}

__global__ __launch_bounds__(SEMI_T) void k_semi_grad(const float* __restrict__ mu, int interleaved, const int64_t* __restrict__ rows,
                                                      int n, int D, int K, Factors f, int kind, int reduction, int groups,
                                                      const float* __restrict__ w, const double* __restrict__ ws,
                                                      float* __restrict__ dmu, double* __restrict__ out, float* loss_io) {
  __shared__ double tot[2 + SEMI_D + SEMI_K + SEMI_D * SEMI_K];            // the sums of the chunks' records
  __shared__ double G[SEMI_D * SEMI_K];                                    // cov: dR/dC
  __shared__ double vc[SEMI_ROWS * SEMI_K];                                // cov: the chunk's centred values, 0 where unlabelled
  __shared__ double red[SEMI_T / 64];
  __shared__ int slot[SEMI_T / 64];
  const int t = threadIdx.x, g = blockIdx.x;
  const bool cov = kind == DVAE_SEMI_COV;
  const int rd = rec_doubles(D, K), used = cov ? rd : 2;
  // the sums of the chunks, in the order of the chunks
  for (int e = t; e < used; e += SEMI_T) {
    double s = 0.;
    for (int k = 0; k < groups; ++k) s += ws[(long)k * rd + e];
    tot[e] = s;
  }
  __syncthreads();
  const double n_lab = tot[0];
  const double inv_n = n_lab > 0. ? 1. / n_lab : 0.;
  double part = 0.;                                                        // cov: this thread's part of R
  for (int p = t; p < D * K; p += SEMI_T) {
    double c = 0.;
    if (cov) {
      const int d = p / K, k = p % K;
      c = tot[2 + D + K + p] * inv_n - (tot[2 + d] * inv_n) * (tot[2 + D + k] * inv_n);
      G[p] = d == k ? 0. : 2. * c;
      if (d != k) part += c * c;
    }
    if (g == 0) out[2 + p] = c;
  }
  if (g == 0) {                                                            // the scalars: lanes, then waves, then thread 0
    part = wave_sum_f64(part);
    if ((t & 63) == 0) red[t >> 6] = part;
    __syncthreads();
    if (t == 0) {
      double r = 0.;
      for (int wv = 0; wv < SEMI_T / 64; ++wv) r += red[wv];
      if (!cov) r = reduction == DVAE_SEMI_MEAN ? tot[1] * inv_n : tot[1];
      out[0] = r;
      out[1] = n_lab;
      if (loss_io) *loss_io = *loss_io + (float)((double)*w * r);
    }
  }
  if (!dmu) return;
  const int c0 = g * SEMI_ROWS, nr = lesser(SEMI_ROWS, n - c0);
  const double wv = (double)*w;
  if (cov) {
    const int i0 = first_labelled(rows, n, slot);
    const long row0 = i0 < n ? rows[i0] : 0;
    for (int i = t; i < nr * K; i += SEMI_T) {
      const int r = i / K, k = i % K;
      const long row = rows[c0 + r];
      const long v = row >= 0 ? (row / f.stride[k]) % f.size[k] : 0, v0 = (row0 / f.stride[k]) % f.size[k];
      vc[i] = row >= 0 ? (double)(v - v0) - tot[2 + D + k] * inv_n : 0.;
    }
    __syncthreads();                                                       // G and vc are written
    for (int i = t; i < nr * D; i += SEMI_T) {
      const int r = i / D, d = i % D;
      double a = 0.;
      for (int k = 0; k < K; ++k) a += G[d * K + k] * vc[r * K + k];
      dmu[(long)c0 * D + i] = rows[c0 + r] >= 0 ? (float)(wv * inv_n * a) : 0.f;
    }
    return;
  }
  const double scale = reduction == DVAE_SEMI_MEAN ? wv * inv_n : wv;
  for (int i = t; i < nr * D; i += SEMI_T) {
    const int r = i / D, d = i % D;
    const long row = rows[c0 + r];
    float out_v = 0.f;
    if (row >= 0 && d < K) {
      const double x = (double)mu[mu_at(interleaved, D, c0 + r, d)];
      const double y = (double)((row / f.stride[d]) % f.size[d]) / (double)f.size[d];
      const double gr = kind == DVAE_SEMI_XENT ? 1. / (1. + exp(-x)) - y : 2. * (x - y);
      out_v = (float)(scale * gr);
    }
    dmu[(long)c0 * D + i] = out_v;
  }
}

bool sizes_ok(long n, int D, int K) {
  return n >= 1 && n <= DVAE_SEMI_MAX_ROWS && K >= 1 && K <= DVAE_SEMI_MAX_K && D >= K && D <= DVAE_SEMI_MAX_D;
}

int chunks(long n) { return (int)((n + SEMI_ROWS - 1) / SEMI_ROWS); }

// 0 when every size and stride is at least 1
int load_factors(const int64_t* sizes, const int64_t* strides, int K, Factors* f) {
  for (int k = 0; k < SEMI_K; ++k) {
    f->size[k] = k < K ? (long)sizes[k] : 1;
    f->stride[k] = k < K ? (long)strides[k] : 1;
    if (f->size[k] < 1 || f->stride[k] < 1) return -1;
  }
  return 0;
}

}  // namespace
}  // namespace dvae

using namespace dvae;

extern "C" {

int dvae_semi_version(void) { return DVAE_SEMI_VERSION; }
const char* dvae_semi_last_error(void) { return last_error(); }

size_t dvae_semi_ws_doubles(long n, int D, int K) {
  if (!sizes_ok(n, D, K)) return 0;
  return (size_t)chunks(n) * (size_t)rec_doubles(D, K);
}

int dvae_semi_partials(const float* mu, int mu_interleaved, const int64_t* rows, long n, int D, int K, const int64_t* sizes,
                       const int64_t* strides, int kind, double* ws, void* stream) {
  DVAE_CHECK_ARG(mu && rows && sizes && strides && ws);
  DVAE_CHECK_ARG(D <= DVAE_SEMI_MAX_D);
  DVAE_CHECK_ARG(K <= DVAE_SEMI_MAX_K);
  DVAE_CHECK_ARG(n <= DVAE_SEMI_MAX_ROWS);
  DVAE_CHECK_ARG(sizes_ok(n, D, K));
  DVAE_CHECK_ARG(mu_interleaved == 0 || mu_interleaved == 1);
  DVAE_CHECK_ARG(kind == DVAE_SEMI_XENT || kind == DVAE_SEMI_L2 || kind == DVAE_SEMI_COV);
  Factors f;
  DVAE_CHECK_ARG(load_factors(sizes, strides, K, &f) == 0);
  hipLaunchKernelGGL(k_semi_partials, dim3(chunks(n)), dim3(SEMI_T), 0, (hipStream_t)stream, mu, mu_interleaved, rows, (int)n, D, K, f,
                     kind, ws);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int dvae_semi_grad(const float* mu, int mu_interleaved, const int64_t* rows, long n, int D, int K, const int64_t* sizes,
                   const int64_t* strides, int kind, int reduction, const float* w, const double* ws, float* dmu, double* out,
                   float* loss_io, void* stream) {
  DVAE_CHECK_ARG(mu && rows && sizes && strides && w && ws && out);
  DVAE_CHECK_ARG(D <= DVAE_SEMI_MAX_D);
  DVAE_CHECK_ARG(K <= DVAE_SEMI_MAX_K);
  DVAE_CHECK_ARG(n <= DVAE_SEMI_MAX_ROWS);
  DVAE_CHECK_ARG(sizes_ok(n, D, K));
  DVAE_CHECK_ARG(mu_interleaved == 0 || mu_interleaved == 1);
  DVAE_CHECK_ARG(kind == DVAE_SEMI_XENT || kind == DVAE_SEMI_L2 || kind == DVAE_SEMI_COV);
  DVAE_CHECK_ARG(reduction == DVAE_SEMI_SUM || reduction == DVAE_SEMI_MEAN);
  Factors f;
  DVAE_CHECK_ARG(load_factors(sizes, strides, K, &f) == 0);
  hipLaunchKernelGGL(k_semi_grad, dim3(chunks(n)), dim3(SEMI_T), 0, (hipStream_t)stream, mu, mu_interleaved, rows, (int)n, D, K, f, kind,
                     reduction, chunks(n), w, ws, dmu, out, loss_io);
  DVAE_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
