// libdvae_mmd_hip.so (include/dvae_mmd_hip.h): the unbiased maximum mean discrepancy MMD_u between a batch of latent samples
// z [B, D] and as many prior samples p [B, D] (InfoVAE / MMD-VAE, Zhao et al. 2019; the regulariser of WAE-MMD) under an RBF or an
// inverse-multiquadric-sum kernel, and its gradient with respect to z, in two launches.  The work is the 3 B^2 pairs (z-z, z-p
// with a gradient; p-p for the value) times D: compute, not bandwidth.
//
// k_mmd_pairs<KIND>.  Workgroup (row tile x, column chunk y): a tile is DVAE_MMD_ROWS rows of z (x < tiles) or of p; a z tile
// meets the 2 B columns [z; p], a p tile the B columns of p; the columns are cut into at most DVAE_MMD_MAX_CGROUPS chunks and a
// workgroup walks its chunk in trips of DVAE_MMD_COLS columns.  Rows and a trip's columns sit in LDS as fp64 (the conversion is
// exact, so every difference a_d - b_d is exact and r^2 never goes through |a|^2 + |b|^2 - 2 a.b) with an ODD row stride: the 32
// lanes of a half wave read 32 different columns at the same d -- 8-byte reads 32 different bank pairs apart -- and ONE row,
// which the LDS broadcasts.  A trip has two phases:
//   pairs   thread t owns column t % COLS and the rows t / COLS, t / COLS + 8: r^2 in fp64, then k and k' from the fp32 r^2 (one
//           exp, or seven v_rcp: no division), k added to the thread's fp64 value sums, c_ij = coefficient * k' stored to LDS;
//   rows    (with a gradient, z tiles) thread (i, d) adds sum_j c_ij (a_id - b_jd) over the trip's columns in order, fp64; c_ij is
//           one word that the lanes of a row share (broadcast), b_jd consecutive words.
// After the last trip the value sums are reduced lanes -> waves -> thread 0 (a fixed tree) into one record, and the gradient
// partials of the chunk go to ws.
//
// k_mmd_finish.  Workgroup 0 adds the value records in a fixed order, writes `out` and adds w MMD_u to *loss_io; with dmu every
// workgroup adds the chunk partials of 256 (row, d) entries in the order of the chunks, scales by w and stores dmu and
// dlv = dmu (z - mu) / 2, one rounding each.
//
// No atomics, no cooperative launch, no workgroup waits on another; every loop bound is a function of the arguments.
#include "../../include/dvae_mmd_hip.h"
#include "common.h"
#include "last_error.h"
#include "table_stats.h"

namespace dvae {

namespace {

#define MMD_T DVAE_MMD_THREADS
#define MMD_ROWS DVAE_MMD_ROWS
#define MMD_COLS DVAE_MMD_COLS
#define MMD_CS (MMD_COLS + 1)                                            // row stride of c in LDS: the rows of a wave on different banks
#define MMD_ITEMS ((MMD_ROWS * DVAE_MMD_MAX_D + MMD_T - 1) / MMD_T)      // (row, d) entries of a tile per thread, at most

static_assert(MMD_T == 256 && MMD_T % 64 == 0, "four waves");
static_assert(MMD_COLS == 32 && MMD_T / MMD_COLS * 2 == MMD_ROWS, "thread t owns column t % 32 and two rows: a half wave is one row");
static_assert(8 * (MMD_ROWS + MMD_COLS) * (DVAE_MMD_MAX_D + 1) + 4 * MMD_ROWS * MMD_CS + 64 <= 64 * 1024, "k_mmd_pairs' LDS");

// WAE's scales of the inverse multiquadric sum
__device__ const float kImqScale[7] = {0.1f, 0.2f, 0.5f, 1.f, 2.f, 5.f, 10.f};
#define MMD_NSCALE 7

__host__ __device__ __forceinline__ int odd_stride(int D) { return D | 1; }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// k and k' (d_a k = k' (a - b)) of one pair from its fp32 r^2.  hp: -1 / h (rbf); cs: C_s = h s (imq)
template <int KIND>
__device__ __forceinline__ void kernel_of(float r2, float hp, const float* cs, float* k, float* kp) {
  if (KIND == DVAE_MMD_RBF) {
    const float e = expf(r2 * hp);
    *k = e;
    *kp = 2.f * hp * e;
  } else {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int s = 0; s < MMD_NSCALE; ++s) {
      const float rc = __builtin_amdgcn_rcpf(cs[s] + r2);
      const float t = cs[s] * rc;
      a += t;
      b += t * rc;
    }
    *k = a;
    *kp = -2.f * b;
  }
}

template <int KIND>
__global__ __launch_bounds__(MMD_T) void k_mmd_pairs(const float* __restrict__ z, const float* __restrict__ p, int B, int D, int tiles,
                                                      int chunk_z, int groups_z, int chunk_p, int groups_p, float hp, float h,
                                                      float coef_zz, float coef_zp, int with_grad, double* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) double mmd_lds[];
  const int Dp = odd_stride(D);
  double* xs = mmd_lds;                                                  // [MMD_ROWS, Dp] the tile's rows
  double* ys = xs + MMD_ROWS * Dp;                                       // [MMD_COLS, Dp] a trip's columns
  double* red = ys + MMD_COLS * Dp;                                      // [8] the waves' value sums
  float* cl = (float*)(red + 8);                                         // [MMD_ROWS, MMD_CS] c_ij of a trip
  const int t = threadIdx.x;
  const bool ztile = (int)blockIdx.x < tiles;
  const int y = blockIdx.y;
  if (!ztile && y >= groups_p) return;                                   // (uniform) a p tile has fewer chunks
  const int r0 = (ztile ? blockIdx.x : blockIdx.x - tiles) * MMD_ROWS;
  const int nr = lesser(MMD_ROWS, B - r0);
  const float* rows = ztile ? z : p;
  // columns: index into [z; p]; a p tile starts at B
  const int chunk = ztile ? chunk_z : chunk_p;
  const int ncols = ztile ? 2 * B : B;
  const int c0 = y * chunk, c1 = lesser(ncols, c0 + chunk);
  const int cbase = ztile ? 0 : B;
  float cs[MMD_NSCALE];
#pragma unroll
  for (int s = 0; s < MMD_NSCALE; ++s) cs[s] = h * kImqScale[s];
  for (int i = t; i < nr * D; i += MMD_T) xs[(i / D) * Dp + i % D] = (double)rows[(long)r0 * D + i];
  const int pj = t % MMD_COLS, pi = t / MMD_COLS;                        // pairs (pi, pj) and (pi + 8, pj)
  const bool grads = ztile && with_grad;
  double same = 0., cross = 0.;                                          // z tile: S_zz, S_zp; p tile: S_pp, nothing
  double acc[MMD_ITEMS];
#pragma unroll
  for (int k = 0; k < MMD_ITEMS; ++k) acc[k] = 0.;
  for (int j0 = c0; j0 < c1; j0 += MMD_COLS) {
    const int nc = lesser(MMD_COLS, c1 - j0);
    __syncthreads();                                                     // xs is written; the trip before is read
    for (int i = t; i < nc * D; i += MMD_T) {
      const int gj = cbase + j0 + i / D;                                 // row of [z; p]
      ys[(i / D) * Dp + i % D] = (double)(gj < B ? z[(long)gj * D + i % D] : p[(long)(gj - B) * D + i % D]);
    }
    __syncthreads();
    const int gj = cbase + j0 + pj;
    const bool jz = gj < B;                                              // a column of z (z tiles only)
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int i = pi + half * (MMD_ROWS / 2);
      float c = 0.f;
      if (i < nr && pj < nc) {
        const double* a = xs + i * Dp;
        const double* b = ys + pj * Dp;
        double r2 = 0.;
        for (int d = 0; d < D; ++d) {
          const double df = a[d] - b[d];
          r2 = fma(df, df, r2);
        }
        float k, kp;
        kernel_of<KIND>((float)r2, hp, cs, &k, &kp);
        const int gi = r0 + i;
        if (ztile && !jz) {
          cross += (double)k;
          c = coef_zp * kp;
        } else if (gi != (ztile ? gj : gj - B)) {                        // the same table: i == j is left out by index
          same += (double)k;
          c = coef_zz * kp;
        }
      }
      cl[i * MMD_CS + pj] = c;
    }
    if (grads) {
      __syncthreads();
#pragma unroll
      for (int k = 0; k < MMD_ITEMS; ++k) {
        const int it = t + k * MMD_T;
        if (it < nr * D) {
          const int i = it / D, d = it % D;
          const double a = xs[i * Dp + d];
          double s = acc[k];
          for (int j = 0; j < nc; ++j) s = fma((double)cl[i * MMD_CS + j], a - ys[j * Dp + d], s);
          acc[k] = s;
        }
      }
    }
  }
  // the value record: lanes, then waves, then thread 0
  same = wave_sum_f64(same);
  cross = wave_sum_f64(cross);
  if ((t & 63) == 0) {
    red[2 * (t >> 6)] = same;
    red[2 * (t >> 6) + 1] = cross;
  }
  __syncthreads();
  if (t == 0) {
    double a = 0., b = 0.;
    for (int w = 0; w < MMD_T / 64; ++w) {
      a += red[2 * w];
      b += red[2 * w + 1];
    }
    double* rec = ws + 2L * ((long)blockIdx.x * groups_z + y);
    rec[0] = a;
    rec[1] = b;
  }
  if (grads) {
    double* part = ws + 4L * tiles * groups_z;                           // [B, groups_z, D]
#pragma unroll
    for (int k = 0; k < MMD_ITEMS; ++k) {
      const int it = t + k * MMD_T;
      if (it < nr * D) part[((long)(r0 + it / D) * groups_z + y) * D + it % D] = acc[k];
    }
  }
}

__global__ __launch_bounds__(MMD_T) void k_mmd_finish(const float* __restrict__ z, const float* __restrict__ mu, int B, int D, int tiles,
                                                       int groups_z, int groups_p, double w, const double* __restrict__ ws,
                                                       float* __restrict__ dmu, float* __restrict__ dlv, double* __restrict__ out,
                                                       float* loss_io) {
  __shared__ double red[3 * MMD_T / 64];
  const int t = threadIdx.x;
  if (blockIdx.x == 0) {                                                 // the value: records in a fixed order
    double zz = 0., zp = 0., pp = 0.;
    const long nrec = 2L * tiles * groups_z;
    for (long r = t; r < nrec; r += MMD_T) {
      const long tile = r / groups_z, y = r % groups_z;
      if (tile < tiles) {
        zz += ws[2 * r];
        zp += ws[2 * r + 1];
      } else if (y < groups_p) {
        pp += ws[2 * r];
      }
    }
    zz = wave_sum_f64(zz);
    zp = wave_sum_f64(zp);
    pp = wave_sum_f64(pp);
    if ((t & 63) == 0) {
      red[3 * (t >> 6)] = zz;
      red[3 * (t >> 6) + 1] = zp;
      red[3 * (t >> 6) + 2] = pp;
    }
    __syncthreads();
    if (t == 0) {
      zz = zp = pp = 0.;
      for (int v = 0; v < MMD_T / 64; ++v) {
        zz += red[3 * v];
        zp += red[3 * v + 1];
        pp += red[3 * v + 2];
      }
      const double b = (double)B;
      const double mmd = B > 1 ? (zz + pp) / (b * (b - 1.)) - 2. * zp / (b * b) : 0.;
      out[0] = w * mmd;
      out[1] = mmd;
      out[2] = zz;
      out[3] = pp;
      out[4] = zp;
      if (loss_io) *loss_io = *loss_io + (float)(w * mmd);
    }
  }
  if (!dmu) return;
  const long i = (long)blockIdx.x * MMD_T + t;                           // entry (row, d)
  if (i >= (long)B * D) return;
  const long row = i / D;
  const int d = (int)(i % D);
  const double* part = ws + 4L * tiles * groups_z + (row * groups_z) * D + d;
  double g = 0.;
  if (B > 1)
    for (int y = 0; y < groups_z; ++y) g += part[(long)y * D];
  g *= w;
  dmu[i] = (float)g;
  if (dlv) dlv[i] = (float)(g * (0.5 * ((double)z[i] - (double)mu[i])));
}

size_t pairs_lds(int D) { return (size_t)(8L * (MMD_ROWS + MMD_COLS) * odd_stride(D) + 64 + 4L * MMD_ROWS * MMD_CS); }

bool sizes_ok(long B, int D) { return B >= 1 && B <= DVAE_MMD_MAX_B && D >= 1 && D <= DVAE_MMD_MAX_D; }

// the tiling of a batch: row tiles per table, column chunks of a z tile and of a p tile
struct Tiling {
  int tiles, groups_z, groups_p;
  long chunk_z, chunk_p;
};

Tiling tiling_of(long B) {
  Tiling g;
  g.tiles = (int)((B + MMD_ROWS - 1) / MMD_ROWS);
  g.groups_z = chunks_of(2 * B, MMD_COLS, DVAE_MMD_MAX_CGROUPS, &g.chunk_z);
  g.groups_p = chunks_of(B, MMD_COLS, DVAE_MMD_MAX_CGROUPS, &g.chunk_p);
  return g;
}

}  // namespace
}  // namespace dvae

using namespace dvae;

extern "C" {

int dvae_mmd_version(void) { return DVAE_MMD_VERSION; }
const char* dvae_mmd_last_error(void) { return last_error(); }

size_t dvae_mmd_ws_doubles(long B, int D) {
  if (!sizes_ok(B, D)) return 0;
  const Tiling g = tiling_of(B);
  return (size_t)(4L * g.tiles * g.groups_z + B * g.groups_z * D);
}

int dvae_mmd_pairs(const float* z, const float* p, long B, int D, int kernel, double h, int with_grad, double* ws, void* stream) {
  DVAE_CHECK_ARG(z && p && ws);
  DVAE_CHECK_ARG(D <= DVAE_MMD_MAX_D);
  DVAE_CHECK_ARG(B <= DVAE_MMD_MAX_B);
  DVAE_CHECK_ARG(sizes_ok(B, D));
  DVAE_CHECK_ARG(kernel == DVAE_MMD_RBF || kernel == DVAE_MMD_IMQ);
  DVAE_CHECK_ARG(h > 0. && h <= 3.0e38);
  const Tiling g = tiling_of(B);
  const double b = (double)B;
  const float coef_zz = B > 1 ? (float)(2. / (b * (b - 1.))) : 0.f, coef_zp = (float)(-2. / (b * b));
  const dim3 grid(2 * g.tiles, g.groups_z);
  const auto kern = kernel == DVAE_MMD_RBF ? k_mmd_pairs<DVAE_MMD_RBF> : k_mmd_pairs<DVAE_MMD_IMQ>;
  hipLaunchKernelGGL(kern, grid, dim3(MMD_T), pairs_lds(D), (hipStream_t)stream, z, p, (int)B, D, g.tiles, (int)g.chunk_z, g.groups_z,
                     (int)g.chunk_p, g.groups_p, (float)(-1. / h), (float)h, coef_zz, coef_zp, with_grad, ws);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int dvae_mmd_finish(const float* z, const float* mu, long B, int D, double w, const double* ws, float* dmu, float* dlv, double* out,
                    float* loss_io, void* stream) {
  DVAE_CHECK_ARG(ws && out);
  DVAE_CHECK_ARG(D <= DVAE_MMD_MAX_D);
  DVAE_CHECK_ARG(B <= DVAE_MMD_MAX_B);
  DVAE_CHECK_ARG(sizes_ok(B, D));
  DVAE_CHECK_ARG(w - w == 0.);                                           // finite
  DVAE_CHECK_ARG(!dlv || (dmu && z && mu));
  const Tiling g = tiling_of(B);
  const int blocks = dmu ? (int)((B * D + MMD_T - 1) / MMD_T) : 1;
  hipLaunchKernelGGL(k_mmd_finish, dim3(blocks), dim3(MMD_T), 0, (hipStream_t)stream, z, mu, (int)B, D, g.tiles, g.groups_z, g.groups_p, w,
                     ws, dmu, dlv, out, loss_io);
  DVAE_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
