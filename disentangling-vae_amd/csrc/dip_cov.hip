// libdvae_dip_hip.so (include/dvae_dip_hip.h): the DIP-VAE regulariser (Kumar et al. 2018) of a batch of posterior means mu [B, D]
// (and, type II, log-variances) -- the biased batch covariance C, R = lambda_od sum_{d != e} C_de^2 + lambda_d sum_d (C_dd - 1)^2
// and dR/dmu, dR/dlogvar -- in two launches.  The shapes are tiny (B D of a few hundred thousand floats at most), so what
// counts is the number of launches and their fixed latency, not bandwidth.
//
// k_dip_moments.  The rows are cut into `groups` equal chunks (at most DVAE_DIP_MAX_GROUPS; above that the chunks grow and a
// workgroup walks its chunk in trips of DVAE_DIP_BLOCK_ROWS rows).  Workgroup (g, y) holds a trip's rows, shifted by
// x0 = mu[0, :] and converted to fp64 first (so the difference is exact), in LDS; its thread t owns ONE entry p = 256 y + t of the
// D x D matrix and, when d <= e, adds (x - x0)_d (x - x0)_e over the rows of the chunk in order, in a register.  The workgroups
// y = 0 also add the D column sums and, with logvar, the D sums of exp(logvar).  One record of 2 D + D D doubles per chunk goes
// to ws (entries d > e are neither written nor read).  The model is the fp64 covariance of latent_pairs.hip
// (libdvae_unsup_hip.so); nothing is shared with it.
//
// k_dip_grad.  One workgroup per chunk again.  Every workgroup adds the records in the order of the chunks -- the same bits of
// C and G in all of them -- and keeps the mean's shift s1 / B (fp64) and G (fp32, both triangles) in LDS; workgroup 0 also
// writes C and the three scalars to `out` and adds R to *loss_io.  With dmu the workgroup then walks its rows: the centred row
// (x - x0) - s1 / B in fp64 (rounding mu - m in fp32 would lose the centred value of a column that sits far from zero), the
// product with G accumulated in fp64 in the order of e, one rounding to fp32 at the store.  G is read as G[e, d]: it is
// symmetric, and the lanes of a wave (consecutive d) then read consecutive LDS words.
//
// No atomics, no cooperative launch, no workgroup waits on another; every loop bound is a function of the arguments.
#include "../../include/dvae_dip_hip.h"
#include "common.h"
#include "last_error.h"
#include "table_stats.h"

namespace dvae {

namespace {

#define DIP_T DVAE_DIP_THREADS
#define DIP_ROWS DVAE_DIP_BLOCK_ROWS

static_assert(DIP_T == 256 && DIP_T % 64 == 0, "four waves");
static_assert(2 * DVAE_DIP_MAX_D <= DIP_T, "threads [0, D) add the column sums, threads [T / 2, T / 2 + D) the exp(logvar) sums");
static_assert(4 * DVAE_DIP_MAX_D * DVAE_DIP_MAX_D + 8 * DVAE_DIP_MAX_D * (DIP_ROWS + 2) <= 160 * 1024, "k_dip_grad's LDS");

// one chunk's record in ws
__host__ __device__ __forceinline__ long rec_doubles(int D) { return 2L * D + (long)D * D; }

__global__ __launch_bounds__(DIP_T) void k_dip_moments(const float* __restrict__ mu, const float* __restrict__ logvar, long B, int D,
                                                       long chunk, double* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) double dip_lds[];       // xs [DIP_ROWS, D]
  double* xs = dip_lds;
  const int t = threadIdx.x, g = blockIdx.x;
  const long c0 = g * chunk, c1 = lesser(B, c0 + chunk);
  const int p = blockIdx.y * DIP_T + t;
  const bool pair = p < D * D && p / D <= p % D;
  const int pd = pair ? p / D : 0, pe = pair ? p % D : 0;
  const bool sums = blockIdx.y == 0;
  const bool col = sums && t < D, ecol = sums && logvar && t >= DIP_T / 2 && t - DIP_T / 2 < D;
  double acc = 0., acc1 = 0.;
  for (long r0 = c0; r0 < c1; r0 += DIP_ROWS) {
    const int nr = (int)lesser((long)DIP_ROWS, c1 - r0);
    __syncthreads();                                                     // the trip before is read
    for (int i = t; i < nr * D; i += DIP_T) xs[i] = (double)mu[r0 * D + i] - (double)mu[i % D];
    __syncthreads();
    if (pair)
      for (int r = 0; r < nr; ++r) acc += xs[r * D + pd] * xs[r * D + pe];
    if (col)
      for (int r = 0; r < nr; ++r) acc1 += xs[r * D + t];
    if (ecol)
      for (int r = 0; r < nr; ++r) acc1 += exp((double)logvar[(r0 + r) * D + (t - DIP_T / 2)]);
  }
  double* rec = ws + g * rec_doubles(D);
  if (pair) rec[2 * D + p] = acc;
  if (col) rec[t] = acc1;
  if (ecol) rec[D + (t - DIP_T / 2)] = acc1;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(DIP_T) void k_dip_grad(const float* __restrict__ mu, const float* __restrict__ logvar, long B, int D,
                                                    long chunk, int groups, double lambda_od, double lambda_d,
                                                    const double* __restrict__ ws, float* __restrict__ dmu, float* __restrict__ dlv,
                                                    double* __restrict__ out, float* loss_io) {
  extern __shared__ __attribute__((aligned(16))) double dip_lds[];
  double* cs = dip_lds;                                                  // [DIP_ROWS, D] centred rows (first: the reduction's scratch)
  double* shift = cs + DIP_ROWS * D;                                     // [D] s1 / B: the mean minus x0
  double* ebar = shift + D;                                              // [D] mean of exp(logvar)
  float* G = (float*)(ebar + D);                                         // [D, D]
  const int t = threadIdx.x, g = blockIdx.x;
  const long rd = rec_doubles(D);
  const double inv_b = 1. / (double)B;
  // the sums of the chunks, in the order of the chunks
  if (t < D) {
    double s = 0.;
    for (int k = 0; k < groups; ++k) s += ws[k * rd + t];
    shift[t] = s * inv_b;
  }
  if (t >= DIP_T / 2 && t - DIP_T / 2 < D) {
    const int d = t - DIP_T / 2;
    double s = 0.;
    if (logvar)
      for (int k = 0; k < groups; ++k) s += ws[k * rd + D + d];
    ebar[d] = s * inv_b;
  }
  __syncthreads();
  double r_od = 0., r_d = 0.;
  for (int p = t; p < D * D; p += DIP_T) {
    const int d = p / D, e = p % D;
    if (d > e) continue;
    double s = 0.;
    for (int k = 0; k < groups; ++k) s += ws[k * rd + 2 * D + p];
    double c = s * inv_b - shift[d] * shift[e];
    double gde;
    if (d == e) {
      c += ebar[d];
      gde = 2. * lambda_d * (c - 1.);
      r_d += (c - 1.) * (c - 1.);
    } else {
      gde = 2. * lambda_od * c;
      r_od += c * c;
    }
    G[d * D + e] = G[e * D + d] = (float)gde;
    if (g == 0) out[3 + d * D + e] = out[3 + e * D + d] = c;
  }
  if (g == 0) {                                                          // the scalars: lanes, then waves, then thread 0
    r_od = wave_sum_f64(r_od);
    r_d = wave_sum_f64(r_d);
    if ((t & 63) == 0) {
      cs[2 * (t >> 6)] = r_od;
      cs[2 * (t >> 6) + 1] = r_d;
    }
    __syncthreads();
    if (t == 0) {
      double a = 0., b = 0.;
      for (int w = 0; w < DIP_T / 64; ++w) {
        a += cs[2 * w];
        b += cs[2 * w + 1];
      }
      a *= 2. * lambda_od;                                               // both triangles
      b *= lambda_d;
      out[0] = a + b;
      out[1] = a;
      out[2] = b;
      if (loss_io) *loss_io = *loss_io + (float)(a + b);
    }
  }
  if (!dmu) return;
  const long c0 = g * chunk, c1 = lesser(B, c0 + chunk);
  const double two_b = 2. * inv_b;
  for (long r0 = c0; r0 < c1; r0 += DIP_ROWS) {
    const int nr = (int)lesser((long)DIP_ROWS, c1 - r0);
    __syncthreads();                                                     // G is written; the trip before (the scalars' scratch) is read
    for (int i = t; i < nr * D; i += DIP_T) cs[i] = ((double)mu[r0 * D + i] - (double)mu[i % D]) - shift[i % D];
    __syncthreads();
    for (int i = t; i < nr * D; i += DIP_T) {
      const int r = i / D, d = i % D;
      double a = 0.;
      for (int e = 0; e < D; ++e) a += (double)G[e * D + d] * cs[r * D + e];
      dmu[r0 * D + i] = (float)(two_b * a);
      if (dlv) dlv[r0 * D + i] = (float)((double)G[d * D + d] * exp((double)logvar[r0 * D + i]) * inv_b);
    }
  }
}

size_t grad_lds(int D) { return (size_t)(8L * D * (DIP_ROWS + 2) + 4L * D * D); }

bool sizes_ok(long B, int D) { return B >= 1 && B <= 2147483647L && D >= 1 && D <= DVAE_DIP_MAX_D; }

}  // namespace
}  // namespace dvae

using namespace dvae;

extern "C" {

int dvae_dip_version(void) { return DVAE_DIP_VERSION; }
const char* dvae_dip_last_error(void) { return last_error(); }

size_t dvae_dip_ws_doubles(long B, int D) {
  if (!sizes_ok(B, D)) return 0;
  long chunk;
  const int groups = chunks_of(B, DVAE_DIP_BLOCK_ROWS, DVAE_DIP_MAX_GROUPS, &chunk);
  return (size_t)(groups * rec_doubles(D));
}

int dvae_dip_moments(const float* mu, const float* logvar, long B, int D, double* ws, void* stream) {
  DVAE_CHECK_ARG(mu && ws);
  DVAE_CHECK_ARG(D <= DVAE_DIP_MAX_D);
  DVAE_CHECK_ARG(sizes_ok(B, D));
  long chunk;
  const int groups = chunks_of(B, DVAE_DIP_BLOCK_ROWS, DVAE_DIP_MAX_GROUPS, &chunk);
  const dim3 grid(groups, (D * D + DIP_T - 1) / DIP_T);
  hipLaunchKernelGGL(k_dip_moments, grid, dim3(DIP_T), (size_t)(8L * DIP_ROWS * D), (hipStream_t)stream, mu, logvar, B, D, chunk, ws);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int dvae_dip_grad(const float* mu, const float* logvar, long B, int D, double lambda_od, double lambda_d, const double* ws,
                  float* dmu, float* dlv, double* out, float* loss_io, void* stream) {
  DVAE_CHECK_ARG(mu && ws && out);
  DVAE_CHECK_ARG(D <= DVAE_DIP_MAX_D);
  DVAE_CHECK_ARG(sizes_ok(B, D));
  DVAE_CHECK_ARG(!dlv || (dmu && logvar));
  long chunk;
  const int groups = chunks_of(B, DVAE_DIP_BLOCK_ROWS, DVAE_DIP_MAX_GROUPS, &chunk);
  static DeviceOnce attr;
  if (attr.first()) {
    (void)hipFuncSetAttribute((const void*)k_dip_grad, hipFuncAttributeMaxDynamicSharedMemorySize, (int)grad_lds(DVAE_DIP_MAX_D));
  }
  hipLaunchKernelGGL(k_dip_grad, dim3(groups), dim3(DIP_T), grad_lds(D), (hipStream_t)stream, mu, logvar, B, D, chunk, groups, lambda_od,
                     lambda_d, ws, dmu, dlv, out, loss_io);
  DVAE_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
