// Per-image scores of a trained model (new: the reference reports only batch means): the per-row reconstruction term of K
// decoded samples per image, and the importance-weighted estimate of log p(x) (Burda et al.) folded over those rows.
// Semantics restated in include/dvae_hip.h (dvae_recon_rows, dvae_iw_loglik).
#include <math.h>
#include "recon_epilogue.h"

namespace dvae {

namespace {

constexpr int RR_THREADS = 256;
constexpr int RR_ROWS = 8;                                 // reconstruction rows per workgroup (the target's reuse factor)
constexpr int RR_SLICE = RR_THREADS;                       // 16-byte quads per column slice: one per thread (1024 elements)

// One workgroup per (image i, RR_ROWS consecutive samples k0 .., column slice c).  Thread t loads quad t of the slice of the
// target ONCE into registers, then the same quad of the workgroup's (up to) RR_ROWS reconstruction rows -- all row loads issued
// before the first use: 8 x 16 bytes in flight per thread -- and adds the row's four element terms in order.  The slice sum of a
// row is the wave sums added in a fixed order; with more than one slice it goes to part[row][c] and k_recon_rows_finish adds the
// slices in order c = 0, 1, ..  The bits of a row's sum depend on row_quads only (not on the image, K or the grid).
__global__ __launch_bounds__(RR_THREADS) void k_recon_rows(const float* __restrict__ recon, const void* __restrict__ target,
                                                           int u8, int K, int kchunks, int nslice, long row_quads, int dist,
                                                           float* __restrict__ part, float* __restrict__ rec_rows) {
  const int tid = threadIdx.x;
  const long wg = blockIdx.x;
  const int c = (int)(wg % nslice);
  const long ik = wg / nslice;
  const long i = ik / kchunks;
  const int k0 = (int)(ik - i * kchunks) * RR_ROWS;
  const int nr = min(RR_ROWS, K - k0);
  const long row0 = i * K + k0;
  const long q = (long)c * RR_SLICE + tid;
  const bool in = q < row_quads;
  // every load unconditional (a lane past the row reads quad 0, rows past nr read the last row; neither is added): the nine
  // 16-byte loads of a thread are issued back to back, without a branch between them
  const long qc = in ? q : 0;
  const f32x4 t = target_quad(target, u8, i * row_quads + qc);
  const f32x4* __restrict__ r4 = reinterpret_cast<const f32x4*>(recon) + row0 * row_quads + qc;
  f32x4 p[RR_ROWS];
#pragma unroll
  for (int r = 0; r < RR_ROWS; ++r) p[r] = r4[(r < nr ? r : nr - 1) * row_quads];
  float acc[RR_ROWS];
#pragma unroll
  for (int r = 0; r < RR_ROWS; ++r) {
    acc[r] = 0.f;
    if (in && r < nr) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float gl, gr;
        acc[r] += recon_elem(p[r][e], t[e], dist, &gl, &gr);
      }
    }
  }
  __shared__ float red[RR_THREADS / 64][RR_ROWS];
  const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int r = 0; r < RR_ROWS; ++r) {
    const float v = wave_sum(acc[r]);
    if (lane == 0) red[wv][r] = v;
  }
  __syncthreads();
  if (tid < nr) {
    const float v = block_sum4_read(red, tid);
    if (nslice == 1) rec_rows[row0 + tid] = v;
    else part[(row0 + tid) * nslice + c] = v;
  }
}

// rec_rows[r] = sum over c in order of part[r][c]
__global__ __launch_bounds__(256) void k_recon_rows_finish(const float* __restrict__ part, long rows, int nslice,
                                                           float* __restrict__ rec_rows) {
  const long r = blockIdx.x * 256L + threadIdx.x;
  if (r >= rows) return;
  float v = 0.f;
  for (int c = 0; c < nslice; ++c) v += part[r * nslice + c];
  rec_rows[r] = v;
}

// One wave per image.  Lane l computes log w of samples b + l (sum over d in order 0 .. D-1); every lane then folds the 64 values
// of the block into the running (max, sum) in sample order (broadcast by __shfl: the lanes hold the same state, no LDS, no
// barrier).  The KL values are written by all lanes.
constexpr int IW_WAVES = 4;

__global__ __launch_bounds__(64 * IW_WAVES) void k_iw_loglik(const float* __restrict__ mu, const float* __restrict__ logvar,
                                                             const float* __restrict__ z, const float* __restrict__ eps,
                                                             const float* __restrict__ rec_rows, long n_img, int nk, int D,
                                                             float log_k, int first, int last, float* __restrict__ state,
                                                             float* __restrict__ loglik, float* __restrict__ kl) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * IW_WAVES + wv;
  if (i >= n_img) return;                                   // (whole waves)
  if (kl) {
    for (int d = lane; d < D; d += 64) {
      const float m = mu[i * D + d], lv = logvar[i * D + d];
      kl[i * D + d] = kl_elem(m, lv);
    }
  }
  if (!state) return;
  float run_m = -INFINITY, run_s = 0.f;
  if (!first) {
    run_m = state[2 * i];
    run_s = state[2 * i + 1];
  }
  const float* __restrict__ lvi = logvar + i * D;
  for (int b = 0; b < nk; b += 64) {
    const int k = b + lane;
    float lw = 0.f;
    if (k < nk) {
      const long row = i * nk + k;
      const float* __restrict__ zr = z + row * D;
      const float* __restrict__ er = eps + row * D;
      float pz = 0.f, qz = 0.f;
      for (int d = 0; d < D; ++d) {
        const float zz = zr[d], e = er[d];
        pz += zz * zz;
        qz += e * e + lvi[d];
      }
      lw = (-rec_rows[row] - 0.5f * pz) + 0.5f * qz;        // -rec + log p(z) - log q(z|x); the log 2pi terms cancel
    }
    const int n = min(64, nk - b);
    for (int j = 0; j < n; ++j) {
      const float v = __shfl(lw, j, 64);
      if (v > run_m) {
        run_s = run_s * expf(run_m - v) + 1.f;
        run_m = v;
      } else {
        run_s += expf(v - run_m);
      }
    }
  }
  if (lane == 0) {
    state[2 * i] = run_m;
    state[2 * i + 1] = run_s;
    if (last) loglik[i] = (run_m + logf(run_s)) - log_k;
  }
}

}  // namespace

long recon_rows_ws_floats(long n_img, int K, long row_elems) {
  const long nslice = (row_elems / 4 + RR_SLICE - 1) / RR_SLICE;
  return nslice > 1 ? n_img * K * nslice : 0;
}

int launch_recon_rows(const float* recon, const void* target, int target_u8, long n_img, int K, long row_elems, int dist,
                      float* ws, float* rec_rows, hipStream_t s) {
  const long row_quads = row_elems / 4;
  const long nslice = (row_quads + RR_SLICE - 1) / RR_SLICE;
  const int kchunks = (K + RR_ROWS - 1) / RR_ROWS;
  const long blocks = n_img * kchunks * nslice;
  if (nslice > 0x7fffffffL || blocks > 0x7fffffffL) {
    set_error("dvae_recon_rows: %ld images x %d samples of %ld elements is too large for one launch", n_img, K, row_elems);
    return -1;
  }
  if (nslice > 1 && !ws) {
    set_error("dvae_recon_rows: rows of %ld elements need a workspace (dvae_recon_rows_ws_floats)", row_elems);
    return -1;
  }
  hipLaunchKernelGGL(k_recon_rows, dim3((unsigned)blocks), dim3(RR_THREADS), 0, s, recon, target, target_u8, K, kchunks,
                     (int)nslice, row_quads, dist, ws, rec_rows);
  DVAE_CHECK_LAUNCH();
  if (nslice > 1) {
    const long rows = n_img * K;
    hipLaunchKernelGGL(k_recon_rows_finish, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, ws, rows, (int)nslice,
                       rec_rows);
    DVAE_CHECK_LAUNCH();
  }
  return 0;
}

int launch_iw_loglik(const float* mu, const float* logvar, const float* z, const float* eps, const float* rec_rows, long n_img,
                     int nk, int D, int K, int first, int last, float* state, float* loglik, float* kl, hipStream_t s) {
  const long blocks = (n_img + IW_WAVES - 1) / IW_WAVES;
  if (blocks > 0x7fffffffL) {
    set_error("dvae_iw_loglik: %ld images is too many for one launch", n_img);
    return -1;
  }
  hipLaunchKernelGGL(k_iw_loglik, dim3((unsigned)blocks), dim3(64 * IW_WAVES), 0, s, mu, logvar, z, eps, rec_rows, n_img, nk, D,
                     logf((float)K), first, last, state, loglik, kl);
  DVAE_CHECK_LAUNCH();
  return 0;
}

}  // namespace dvae
